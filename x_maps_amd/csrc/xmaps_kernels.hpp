// xmaps_kernels.hpp -- gfx950 (MI355X / CDNA4) device code for the X-maps hot path.
//
// Three kernels per frame (no memset, no host round trip):
//   K0 k_minmax   : frame extrema of t (x_maps_disparity.py:12-13)  -- pure streaming reduction
//   K1 k_scatter  : per event: rectify-LUT gather (cam_proj_calibration.py:277-281) -> FP64 time
//                   normalise + rint (x_maps_disparity.py:16-19) -> X-map gather (:25) -> int16
//                   disparity + inlier masks (:23-29) -> last-writer-wins scatter
//                   (cam_proj_calibration.py:299-303 / 312-317) as ONE 64-bit atomic max
//   K2 k_frame_*  : per output pixel: 7x7 max (cv2.dilate) composed with the nearest remap
//                   (disp_to_depth.py:86-95) -> depth (disp_to_depth.py:46-63) -> u8 normalise
//                   (:7-21) -> Turbo BGR + white mask (:24-43)
//
// Last-writer-wins without a clear: every cell of the disparity frame holds a packed key
//   [63]=0 | frame tag:19 | event index:28 | disparity:16
// and K1 does atomic max.  Inside a frame the largest event index wins (= NumPy's fancy-assignment
// order); keys of older frames carry a smaller tag, lose every max and are ignored by K2, so the
// 9-56 MB frame is never zero-filled.  The tag lives in device memory (SlotState) so that the same
// launches can be replayed from a hipGraph.
//
// This is gather/scatter + integer work: no MFMA.  What matters is coalesced event reads, L2-resident
// tables, fire-and-forget atomics and enough waves in flight to hide three dependent memory latencies.
//
// The device code is split by kernel; this file only gathers it (in the order the definitions depend on each other):
#pragma once
#include "xmaps_common.hpp"     // device ABI (DevTables, SlotState, FrameDesc, keys), time codecs, TimeNorm, per-event arithmetic, XM_ABLATE
#include "xmaps_k0.hpp"         // K0: frame extrema of t
#include "xmaps_k1direct.hpp"   // K1, one thread per event
#include "xmaps_k1tiles.hpp"    // K1 on event tiles (LDS bands and slots)
#include "xmaps_k2.hpp"         // K2: every frame kernel and its table builders
#include "xmaps_stage.hpp"      // stage and debug kernels, point cloud
#include "xmaps_xmapbuild.hpp"  // X-map builder (setup time)
#include "xmaps_rigmaps.hpp"    // a rig's rectification maps + remap in front of it (setup time): calibration.py's NumPy, bit for bit
#include "xmaps_filters.hpp"    // frame event filters, pause detection
#include "xmaps_eval.hpp"       // evaluation metrics
#include "xmaps_slots.hpp"      // slot reset, redo preparation
#include "xmaps_eslinit.hpp"    // the ESL-init baseline: disparity search per rectified / per camera pixel (brings xmaps_surface.hpp)
#include "xmaps_mc3d.hpp"       // the MC3D baseline: median, projector-column window search and depth per camera pixel
#include "xmaps_esloptim.hpp"   // the ESL depth optimisation: one bounded scalar minimisation per camera pixel
#include "xmaps_eslfilter.hpp"  // the ESL filters behind it: bilateral filter and TV denoiser (split Bregman around lsqr)
#include "xmaps_evaltable.hpp"  // the evaluation table's scorer: combine, median, the metrics of every (method, scan) cell
// (included by xmaps_hip.hip behind the ingest, whose frame descriptors it reads:)
//       "xmaps_framesurface.hpp"  frames of events -> camera time surfaces: winners by integer atomics, one store per pixel
//       "xmaps_framecloud.hpp"    frames of events -> per-event point clouds: codes per event, a scan, a stable compaction
//       "xmaps_evt3enc.hpp"       frames of events -> EVT 3.0 words: run starts per chain, counts per 64 events, a scan, a stable emit
//       "xmaps_timecal.hpp"       projector time-map calibration: accumulate, mean, corners, projective warp, fill along rows
// (and behind the decoders:)
//       "xmaps_exttrigger.hpp"    EXT_TRIGGER words -> trigger records; the triggered frames' append (p == 1 compaction + trigger remap)
//       "xmaps_trigfilter.hpp"    the triggered frames' two filters: the activity rule inside the append (first pass, sequential
//                                 judge, count, write + retire), the frame event filters on a run of ready frames (blockIdx.y = frame)
