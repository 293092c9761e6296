// xm_api_evt3enc.hpp -- C-ABI: a group of frames of EventCD records -> the EVT 3.0 words of every frame, in one device call
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and what each pass leaves behind: ../xmaps_evt3enc.hpp.  The ingest runs the same launches as a stage of its frame
// stream (xm_ingest_launch.hpp, xm_api_ingest.hpp).
#pragma once

static_assert(sizeof(xm_evt3_record_stats) == sizeof(EncStats), "xm_evt3_record_stats is what k_enc_scan writes");

extern "C" {

int xm_frames_to_evt3_words(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_vectors, int mem,
                            uint16_t* words_out, xm_evt3_record_stats* stats_out) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = group_args(n_frames, mem, nullptr, "frames"))) return rc;
  if (!offsets_host) return fail(XM_ERR_INVALID, "NULL argument");
  FrameSpans sp;
  // (a frame's 4 * n words are counted in 32 bits)
  if ((rc = frame_spans(eventcd16, offsets_host, n_frames, mem, 1ull << 30, "group too large (it holds at most 2^30 - 1 events)", &sp))) return rc;
  const u64 ev0 = sp.ev0, n_total = sp.n_total;
  if (n_total && !words_out) return fail(XM_ERR_INVALID, "NULL argument");
  const bool host = mem == XM_MEM_HOST;
  XM_ENTER(h);
  FrameRecordScratch& sc = h->frecord;
  const size_t n = (size_t)n_frames;
  const size_t n_seg = (size_t)(n_total / 64) + n;  // >= the frames' ceil(n / 64) together
  Slot& s = pick_slot(h);
  hipStream_t stream = s.stream;

  // scratch: grown when a larger group arrives -- only once nothing that was enqueued earlier can still be using it
  const std::initializer_list<BufNeed> needs = {{sc.code, (size_t)n_total * 2},
                                                {sc.cnt, n_seg * sizeof(uint2)},
                                                {sc.off, n_seg * 4},
                                                {sc.stats, n * sizeof(EncStats)},
                                                {sc.in, host ? (size_t)n_total * 16 : 0},
                                                {sc.out, host ? (size_t)n_total * 8 : 0}};
  rc = sc.order.enter(stream, any_grows(needs), false, [&] { return reserve_all(needs); }, [&] { return (int)XM_OK; });
  if (rc) return rc;

  const uint4* d_ev;
  if ((rc = frame_records(eventcd16, sp, host, sc.in, stream, &d_ev))) return rc;
  uint16_t* d_words = host ? (uint16_t*)sc.out.p : words_out;
  EncStats* d_stats = (EncStats*)sc.stats.p;
  const u32 max_blocks = frame_max_chunk_blocks("XM_ENC_MAX_BLOCKS");
  u64 seg = 0;
  for (size_t f0 = 0; f0 < n; f0 += ENC_GROUP) {  // launch sequences of at most ENC_GROUP frames
    const unsigned nf = (unsigned)std::min<size_t>(ENC_GROUP, n - f0);
    EncArgs a{};
    a.ev = d_ev;
    const u64 seq_max = frame_seq_fill(offsets_host, ev0, f0, nf, a.first, a.n);
    for (unsigned k = 0; k < nf; ++k) {
      a.seg0[k] = (u32)seg;
      seg += ((u64)a.n[k] + 63) / 64;
    }
    a.max_words = 0xffffffffu;
    a.code = (uint16_t*)sc.code.p;
    a.cnt = (uint2*)sc.cnt.p;
    a.off = (u32*)sc.off.p;
    a.stats = d_stats + f0;
    a.words = d_words;
    a.use_vectors = use_vectors ? 1 : 0;
    a.max_chunk_blocks = max_blocks;
    launch_frame_records(a, nf, seq_max, stream);
    HIP_TRY(hipGetLastError());
  }
  s.order.note_eager();

  if (!host) {
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(EncStats), hipMemcpyDeviceToDevice, stream));
    return sc.order.leave_async(stream);
  }
  std::vector<xm_evt3_record_stats> st(n);
  HIP_TRY(hipMemcpyAsync(st.data(), d_stats, n * sizeof(EncStats), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sc.order.leave_sync();
  for (size_t i = 0; i < n; ++i) {  // only the valid words of every frame cross the bus
    const size_t w0 = (size_t)(offsets_host[i] - ev0) * 4;
    if (st[i].n_words) HIP_TRY(hipMemcpyAsync(words_out + w0, d_words + w0, (size_t)st[i].n_words * 2, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (stats_out) std::memcpy(stats_out, st.data(), n * sizeof(xm_evt3_record_stats));
  return XM_OK;
}

}  // extern "C"
