// xm_api_evt3.hpp -- C-ABI: EVT 3.0 / EVT 2.0 / EVT 2.1 words and DAT records -> EventCD records on the device (xmaps_evt3.hpp,
// xmaps_evt2.hpp, xmaps_evt21.hpp, xmaps_dat.hpp; xmaps_evt.hpp).  One decoder object for the four formats (`format`): same
// buffers, same state record, same three launches.  Straight into the ingest: xm_ingest_push_evt3 / _evt2 / _evt21 / _dat
// (xm_api_ingest.hpp), which enqueue the same launches (evt3_enqueue) from the ingest's copy side.
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

struct xm_evt3 {
  xm_handle* h = nullptr;
  int device = 0;  // (kept here: the decoder may be destroyed after its handle)
  Stream stream;
  size_t max_words = 0, max_events = 0;
  int format = 3;                // 3: 16-bit EVT 3.0 words; 2: 32-bit EVT 2.0 words; EVT_FMT_21: 64-bit EVT 2.1 words; EVT_FMT_DAT: 8-byte DAT records
  size_t word_bytes = 2;
  PinnedMem<uint16_t> h_words;   // pinned staging (max_words * word_bytes)
  DevMem<uint16_t> d_words;
  DevMem<Evt3Scan> d_agg;
  DevMem<Evt3State> d_state;     // [2]: in / out, swapped per chunk
  PinnedMem<Evt3State> h_state;  // pinned: the chunk's event count comes back here
  DevMem<uint4> d_out;           // records of the last xm_evt3_decode
  int cur = 0;
  int wait_tb = 0;               // xm_evt3_wait_for_time_base: events in front of the stream's first TIME_HIGH word are not emitted
  int legacy_halves = 0;         // xm_evt21_set_legacy_halves: each 64-bit word is stored HIGH half first
  int emit_by_word = 1;          // EVT 2.1: k_evt21_emit_words, the faster one (profiles/evt21.md); "XM_EVT21_EMIT_BY_WORD" = 0: k_evt21_emit
  // EXT_TRIGGER extraction (xm_evt_set_ext_triggers, xm_api_exttrigger.hpp); max_triggers = 0: off, nothing below is allocated
  size_t max_triggers = 0;
  DevMem<u32> d_trig_counts;     // per block of the chunk, + the chunk's total behind them
  DevMem<uint4> d_trig;          // the chunk's records (xm_ext_trigger)
  PinnedMem<u32> h_trig_n;       // the chunk's total comes back here
  PinnedMem<uint4> h_trig;       // records of the last successful decode
  size_t n_trig = 0;
};

static_assert(sizeof(Evt2Scan) <= sizeof(Evt3Scan), "the decoders share the aggregates' buffer (d_agg)");
static_assert(sizeof(Evt21Scan) <= sizeof(Evt3Scan), "the decoders share the aggregates' buffer (d_agg)");
static_assert(sizeof(DatScan) <= sizeof(Evt3Scan), "the decoders share the aggregates' buffer (d_agg)");

constexpr int EVT_FMT_21 = 21, EVT_FMT_DAT = 100;  // (xm_evt3::format beside 3 and 2)

namespace {

// xm_api_exttrigger.hpp: the two extraction launches behind the chunk's emit kernel (+ the copy of their total), and the
// download of the records once the chunk is kept
int evt_ext_enqueue(xm_evt3* d, u32 n, u32 nb, hipStream_t stream);
int evt_ext_collect(xm_evt3* d, hipStream_t stream);

const char* evt_format_name(int format) {
  return format == 3 ? "EVT 3.0 words" : format == 2 ? "EVT 2.0 words" : format == EVT_FMT_21 ? "EVT 2.1 words" : "DAT records";
}

// words (host) -> records at `out` (device, room for out_cap) enqueued on `stream`; the chunk's event count is left in
// d->d_state[d->cur ^ 1].n_events (device memory) -- evt3_commit() flips `cur` once the caller has decided to keep the chunk
// count_out (device, may be NULL): the chunk's event count once more, in a cell of the caller's (the state record's copy is
// overwritten two chunks later -- too soon for a consumer on another stream)
int evt3_enqueue(xm_evt3* d, const void* words_host, size_t n_words, bool pinned, uint4* out, size_t out_cap, hipStream_t stream,
                 u32* count_out = nullptr) {
  if (n_words > d->max_words) return fail(XM_ERR_TOO_MANY, "chunk of %zu words exceeds max_words %zu", n_words, d->max_words);
  if (!pinned) {  // pageable memory: through the pinned staging buffer, once its previous chunk has been copied out of it
    HIP_TRY(hipStreamSynchronize(stream));
    memcpy(d->h_words, words_host, n_words * d->word_bytes);
  }
  HIP_TRY(hipMemcpyAsync(d->d_words, pinned ? words_host : (const void*)d->h_words, n_words * d->word_bytes, hipMemcpyHostToDevice, stream));
  const u32 n = (u32)n_words, nb = (u32)grid_for(n_words, EVT_PER_BLOCK);
  Evt3State* st_in = d->d_state + d->cur;
  Evt3State* st_out = d->d_state + (d->cur ^ 1);
  if (d->format == 2) {
    const u32* w32 = reinterpret_cast<const u32*>(d->d_words.get());
    Evt2Scan* agg = reinterpret_cast<Evt2Scan*>(d->d_agg.get());
    hipLaunchKernelGGL(k_evt2_aggregate, dim3(nb), dim3(EVT_THREADS), 0, stream, w32, n, agg);
    hipLaunchKernelGGL(k_evt2_prefix, dim3(1), dim3(EVT_THREADS), 0, stream, nb, agg, (const Evt3State*)st_in, st_out, count_out, d->wait_tb);
    hipLaunchKernelGGL(k_evt2_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, w32, n, (const Evt2Scan*)agg, (const Evt3State*)st_in, out,
                       (u32)std::min<size_t>(out_cap, 0xffffffffu), d->wait_tb);
    HIP_TRY(hipGetLastError());
    return XM_OK;
  }
  if (d->format == EVT_FMT_21) {
    const unsigned long long* w64 = reinterpret_cast<const unsigned long long*>(d->d_words.get());
    Evt21Scan* agg = reinterpret_cast<Evt21Scan*>(d->d_agg.get());
    const u32 cap = (u32)std::min<size_t>(out_cap, 0xffffffffu);
    hipLaunchKernelGGL(k_evt21_aggregate, dim3(nb), dim3(EVT_THREADS), 0, stream, w64, n, agg, d->legacy_halves);
    hipLaunchKernelGGL(k_evt21_prefix, dim3(1), dim3(EVT_THREADS), 0, stream, nb, agg, (const Evt3State*)st_in, st_out, count_out, d->wait_tb);
    if (d->emit_by_word)
      hipLaunchKernelGGL(k_evt21_emit_words, dim3(nb), dim3(EVT_THREADS), 0, stream, w64, n, (const Evt21Scan*)agg, (const Evt3State*)st_in, out, cap,
                         d->wait_tb, d->legacy_halves);
    else
      hipLaunchKernelGGL(k_evt21_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, w64, n, (const Evt21Scan*)agg, (const Evt3State*)st_in, out, cap,
                         d->wait_tb, d->legacy_halves);
    HIP_TRY(hipGetLastError());
    return XM_OK;
  }
  if (d->format == EVT_FMT_DAT) {
    const unsigned long long* r64 = reinterpret_cast<const unsigned long long*>(d->d_words.get());
    DatScan* agg = reinterpret_cast<DatScan*>(d->d_agg.get());
    hipLaunchKernelGGL(k_dat_aggregate, dim3(nb), dim3(EVT_THREADS), 0, stream, r64, n, agg);
    hipLaunchKernelGGL(k_dat_prefix, dim3(1), dim3(EVT_THREADS), 0, stream, nb, agg, (const Evt3State*)st_in, st_out, count_out);
    hipLaunchKernelGGL(k_dat_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, r64, n, (const DatScan*)agg, (const Evt3State*)st_in, out,
                       (u32)std::min<size_t>(out_cap, 0xffffffffu));
    HIP_TRY(hipGetLastError());
    return XM_OK;
  }
  hipLaunchKernelGGL(k_evt3_aggregate, dim3(nb), dim3(EVT_THREADS), 0, stream, (const uint16_t*)d->d_words, n, d->d_agg);
  hipLaunchKernelGGL(k_evt3_prefix, dim3(1), dim3(EVT_THREADS), 0, stream, (const uint16_t*)d->d_words, nb, d->d_agg, (const Evt3State*)st_in, st_out,
                     count_out, d->wait_tb);
  hipLaunchKernelGGL(k_evt3_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, (const uint16_t*)d->d_words, n, (const Evt3Scan*)d->d_agg,
                     (const Evt3State*)st_in, out, (u32)std::min<size_t>(out_cap, 0xffffffffu), d->wait_tb);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// the synchronous form: *n_events once the count is back (synchronises the stream)
// ext: the chunk's EXT_TRIGGER records as well, when the decoder has them on (the synchronous decode entries; the ingest's does not)
int evt3_run(xm_evt3* d, const void* words_host, size_t n_words, bool pinned, uint4* out, size_t out_cap, hipStream_t stream, size_t* n_events,
             bool ext = false) {
  *n_events = 0;
  if (!n_words) {
    if (ext) d->n_trig = 0;  // (an empty chunk holds no trigger)
    return XM_OK;
  }
  int rc = evt3_enqueue(d, words_host, n_words, pinned, out, out_cap, stream);
  if (rc) return rc;
  ext = ext && d->max_triggers;
  if (ext) {
    rc = evt_ext_enqueue(d, (u32)n_words, (u32)grid_for(n_words, EVT_PER_BLOCK), stream);
    if (rc) return rc;
  }
  HIP_TRY(hipMemcpyAsync(d->h_state, d->d_state + (d->cur ^ 1), sizeof(Evt3State), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *n_events = (size_t)d->h_state->n_events;
  // Too many events for `out`: the decoder's state is NOT advanced (st_in is still current), so the caller can decode the same
  // chunk again into a larger buffer or in halves; the records written so far are a truncated prefix and must not be used.
  if (*n_events > out_cap) return fail(XM_ERR_TOO_MANY, "the chunk decodes to %zu events, room for %zu (decoder state unchanged: decode it again in smaller pieces)", *n_events, out_cap);
  if (ext) {  // too many trigger words for the records' buffer: the same contract
    if (*d->h_trig_n > d->max_triggers) return fail(XM_ERR_TOO_MANY, "the chunk holds %u trigger words, room for %zu (decoder state unchanged: decode it again in smaller pieces)", *d->h_trig_n, d->max_triggers);
    rc = evt_ext_collect(d, stream);
    if (rc) return rc;
  }
  d->cur ^= 1;
  return XM_OK;
}

}  // namespace

extern "C" {

static int evt_create(xm_handle* h, int format, size_t max_words, size_t max_events, xm_evt3** out) {
  if (!h || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  XM_ENTER(h);
  Owned<xm_evt3, xm_evt3_destroy> d(new (std::nothrow) xm_evt3());
  if (!d) return fail(XM_ERR_NOMEM, "out of host memory");
  d->h = h;
  d->device = h->cfg.device;
  d->format = format;
  d->word_bytes = format == 3 ? 2 : format == 2 ? 4 : 8;
  d->max_words = max_words ? max_words : (size_t)1 << 20;
  d->max_events = max_events ? max_events : (format == 3 ? 2 : format == EVT_FMT_21 ? 4 : 1) * d->max_words;
  if (d->max_words >= 0x7fffffffull || d->max_events >= 0x7fffffffull) return fail(XM_ERR_INVALID, "max_words and max_events must be < 2^31");
  if (format == EVT_FMT_21 && d->max_words >= ((size_t)1 << 27))  // (a word is up to 32 events and a chunk's event counts are u32)
    return fail(XM_ERR_INVALID, "max_words must be < 2^27 for EVT 2.1");
  if (const char* e = dbg_opt("XM_EVT21_EMIT_BY_WORD")) d->emit_by_word = e[0] == '1';
  const size_t nb = grid_for(d->max_words, EVT_PER_BLOCK);
  const size_t n16 = d->max_words * d->word_bytes / sizeof(uint16_t);
  HIP_TRY(d->stream.create(hipStreamNonBlocking));
  HIP_TRY(d->h_words.alloc(n16, hipHostMallocDefault));
  HIP_TRY(d->h_state.alloc(1, hipHostMallocDefault));
  HIP_TRY(d->d_words.alloc(n16, 64));
  HIP_TRY(d->d_agg.alloc(nb + 1));
  HIP_TRY(d->d_state.alloc(2));
  HIP_TRY(hipMemsetAsync(d->d_state, 0, 2 * sizeof(Evt3State), d->stream));  // (on the decoder's stream: it does not wait for the default one)
  HIP_TRY(hipStreamSynchronize(d->stream));
  HIP_TRY(d->d_out.alloc(d->max_events));
  *out = d.release();
  return XM_OK;
}

int xm_evt3_create(xm_handle* h, size_t max_words, size_t max_events, xm_evt3** out) { return evt_create(h, 3, max_words, max_events, out); }
int xm_evt2_create(xm_handle* h, size_t max_words, size_t max_events, xm_evt3** out) { return evt_create(h, 2, max_words, max_events, out); }
int xm_evt21_create(xm_handle* h, size_t max_words, size_t max_events, xm_evt3** out) { return evt_create(h, EVT_FMT_21, max_words, max_events, out); }
int xm_dat_create(xm_handle* h, size_t max_words, size_t max_events, xm_evt3** out) { return evt_create(h, EVT_FMT_DAT, max_words, max_events, out); }

void xm_evt3_destroy(xm_evt3* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  delete d;
}

int xm_evt3_wait_for_time_base(xm_evt3* d, int on) {
  if (!d) return fail(XM_ERR_INVALID, "NULL argument");
  d->wait_tb = on ? 1 : 0;
  return XM_OK;
}

int xm_evt21_set_legacy_halves(xm_evt3* d, int on) {
  if (!d) return fail(XM_ERR_INVALID, "NULL argument");
  if (d->format != EVT_FMT_21) return fail(XM_ERR_INVALID, "this decoder was created for %s", evt_format_name(d->format));
  d->legacy_halves = on ? 1 : 0;
  return XM_OK;
}

int xm_evt3_reset(xm_evt3* d) {
  if (!d) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipStreamSynchronize(d->stream));
  HIP_TRY(hipMemsetAsync(d->d_state, 0, 2 * sizeof(Evt3State), d->stream));  // (a memset on the default stream could be overtaken by the next chunk's kernels)
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->cur = 0;
  d->n_trig = 0;
  return XM_OK;
}

static int evt_decode(xm_evt3* d, int format, const void* words_host, size_t n_words, const void** events_dev, size_t* n_events) {
  if (!d || (n_words && !words_host) || !n_events) return fail(XM_ERR_INVALID, "NULL argument");
  if (d->format != format) return fail(XM_ERR_INVALID, "this decoder was created for %s", evt_format_name(d->format));
  HIP_TRY(hipSetDevice(d->device));
  if (events_dev) *events_dev = d->d_out;
  return evt3_run(d, words_host, n_words, false, d->d_out, d->max_events, d->stream, n_events, true);
}

int xm_evt3_decode(xm_evt3* d, const uint16_t* words_host, size_t n_words, const void** events_dev, size_t* n_events) {
  return evt_decode(d, 3, words_host, n_words, events_dev, n_events);
}
int xm_evt2_decode(xm_evt3* d, const uint32_t* words_host, size_t n_words, const void** events_dev, size_t* n_events) {
  return evt_decode(d, 2, words_host, n_words, events_dev, n_events);
}
int xm_evt21_decode(xm_evt3* d, const uint64_t* words_host, size_t n_words, const void** events_dev, size_t* n_events) {
  return evt_decode(d, EVT_FMT_21, words_host, n_words, events_dev, n_events);
}
int xm_dat_decode(xm_evt3* d, const void* records_host, size_t n_records, const void** events_dev, size_t* n_events) {
  return evt_decode(d, EVT_FMT_DAT, records_host, n_records, events_dev, n_events);
}

}  // extern "C"
