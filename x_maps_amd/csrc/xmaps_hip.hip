// xmaps_hip.hip -- host side of libxmaps_hip.so: the C-ABI declared in include/xmaps.h.
// Written for MI355X (gfx950) only: build with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared xmaps_hip.hip -o libxmaps_hip.so
// -ffp-contract=off keeps the time normalisation (divide, multiply, rint) unfused = bit-exact with NumPy.
// The device side, one header per kernel (each includes what it needs; xmaps_geometry.hpp, standard C++ only, holds the
// constants and the LDS layouts they share with the host's plan):
#include "xmaps_kernels.hpp"        // common ABI, K0, K1 direct / event tiles, K2, stage, X-map builder, rig maps, filters, eval, slots
#include "xmaps_k1cols.hpp"         // K1 on column tiles + the boundary pass
#include "xmaps_k1own.hpp"          // K1 on owner tiles
#include "xmaps_k2pipe.hpp"         // pipelined K2 on the u16 frame
#include "xmaps_ingest.hpp"         // device-side ingest: activity filter, frame segmentation
#include "xmaps_ingest_filter.hpp"  // ... the frame event filters as a stage of it
#include "xmaps_evt3.hpp"           // EVT 3.0 decoder (xmaps_evt.hpp: what it shares with the next three)
#include "xmaps_evt2.hpp"           // EVT 2.0 decoder
#include "xmaps_evt21.hpp"          // EVT 2.1 decoder
#include "xmaps_dat.hpp"            // DAT (version 2, CD) decoder
#include "xmaps_exttrigger.hpp"     // EXT_TRIGGER words -> trigger records behind the decoders' emit; the triggered frames' append
#include "xmaps_trigfilter.hpp"     // ... their two filters: the activity rule inside the append, the frame event filters on runs of frames
#include "xmaps_surface.hpp"        // time surfaces -> depth maps + point clouds
#include "xmaps_framesurface.hpp"   // frames of events -> camera time surfaces (the group entry and the ingest's surface stage)
#include "xmaps_framecloud.hpp"     // frames of events -> per-event point clouds (the group entry and the ingest's cloud stage)
#include "xmaps_evt3enc.hpp"        // frames of events -> EVT 3.0 words (the group entry and the ingest's record stage)
#include "xmaps_timecal.hpp"        // projector time-map calibration: white-frame time surfaces -> the projector-space time map

#include <hip/hip_ext.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <limits>
#include <map>
#include <memory>
#include <algorithm>
#include <new>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/xmaps.h"

using namespace xm;

// The host side is one translation unit, split by concern (each file closes the namespaces / linkage blocks it opens):
#include "host/xm_plan.hpp"         // the rig plan and the path / launch-shape rules (standard C++ only)
#include "host/xm_queue.hpp"        // the host threads' job queues and first-error latches (standard C++ only)
#include "host/xm_agree.hpp"        // the agreement among a sharded handle's device threads (standard C++ only)
#include "host/xm_res.hpp"          // owners of device / pinned memory, streams and events (RAII)
#include "host/xm_slot_order.hpp"   // where a slot's last work ran; the only code that orders a stream or the host behind it (standard C++ only)
#include "host/xm_scratch_order.hpp"  // how the calls on a handle's per-entry scratch follow each other (standard C++ only)
#include "host/xm_host.hpp"         // errors, slots, launch workers, the handle (RigPlan + owners + run-time state), launch macros
#include "host/xm_launch.hpp"       // launch helpers of every kernel variant
#include "host/xm_own_plan.hpp"     // owner-tile tables (host analysis in xm_create)
#include "host/xm_k2_live.hpp"      // the frame quads the column tiles can ever write -> the pipelined K2's live-slot masks (standard C++ only)
#include "host/xm_enqueue.hpp"      // path selection + the launches of one frame
#include "host/xm_batch.hpp"        // multi-frame launches (groups)
#include "host/xm_workers.hpp"      // redo of failed shortcuts, launch workers, single-frame entry
#include "host/xm_create.hpp"       // the stages of xm_create
#include "host/xm_api_engine.hpp"   // xm_create .. xm_process_batch, adaptive batching
#include "host/xm_api_graph.hpp"    // hipGraph batches
#include "host/xm_api_stage.hpp"    // debug + stage API
#include "host/xm_api_shard.hpp"    // shards (multi-GPU)
#include "host/xm_shard_peers.hpp"  // how a rank reaches its peers (RCCL at run time, agreements, virtual ranks); the two shard exchanges, once
#include "host/xm_api_sharded.hpp"  // one frame over several GPUs of one process: the devices, their threads, the frame's three steps
#include "host/xm_api_shardcomm.hpp"  // one rank of a frame sharded over several processes: argument checks + the same exchanges
#include "host/xm_api_filters.hpp"  // frame event filters, pause detection
#include "host/xm_api_activity.hpp" // the activity filter alone; its device state (shared with the ingest)
#include "host/xm_api_evt3.hpp"     // EVT 3.0 / 2.0 / 2.1 / DAT decoder on the device
#include "host/xm_api_exttrigger.hpp"  // ... its EXT_TRIGGER records; frames cut at them (xm_trigger_cut.hpp: the rule, standard C++ only)
#include "host/xm_ring_tag.hpp"     // the ingest's per-frame output rings: entry and tag arithmetic (standard C++ only)
#include "host/xm_ingest_state.hpp" // device-side ingest: its state by owning thread, the jobs its threads hand each other
#include "host/xm_ingest_out.hpp"   // ... the out side (result copies, sequence numbers) and the frame pool
#include "host/xm_ingest_launch.hpp"  // ... the launch and copy sides (packets, verdicts, frames), the caller's door to them
#include "host/xm_ingest_create.hpp"  // ... the stages of xm_ingest_create
#include "host/xm_api_ingest.hpp"   // ... its C entry points (records, and EVT words through the decoder)
#include "host/xm_api_misc.hpp"     // X-map builder, evaluation metrics, memory helpers
#include "host/xm_api_rigmaps.hpp"  // a rig's rectification maps, time map and X-map: the table builders' device path
#include "host/xm_group.hpp"        // the skeleton of the group objects below: create / destroy, argument check, staging, dtype dispatch
#include "host/xm_api_surface.hpp"  // a group of camera time surfaces -> depth maps + point clouds (the evaluation caller's entry)
#include "host/xm_api_framesurface.hpp"  // a group of frames of events -> camera time surfaces: what joins the live half to the entries around it
#include "host/xm_api_framecloud.hpp"    // a group of frames of events -> per-event point clouds: the live half's 3-D output
#include "host/xm_api_evt3enc.hpp"       // a group of frames of events -> EVT 3.0 words: the way out for the events themselves
#include "host/xm_api_eslinit.hpp"  // the ESL-init baseline on the same surfaces: depth_init maps, disparity_init alone
#include "host/xm_api_mc3d.hpp"     // the MC3D baseline on the same surfaces
#include "host/xm_api_esloptim.hpp" // the ESL depth optimisation behind ESL-init: depth_optim maps
#include "host/xm_api_eslfilter.hpp" // the bilateral filter and the TV denoiser behind it: depth_optim_filtered maps
#include "host/xm_api_evaltable.hpp" // the evaluation table's scorer: ground truth + every method's maps -> the cells of Table 1
#include "host/xm_api_timecal.hpp"  // the projector time-map calibration: accumulate, mean, corners, warp, fill
