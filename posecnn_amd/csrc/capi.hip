// C-ABI housekeeping entry points of libposecnn_hip.so (see include/posecnn_hip.h).
#include "pcnn_common.h"

// 3: the two entry points of the pruned ADD-S search are gone
// 4: the mesh rasteriser (pcnn_render_workspace_size, pcnn_render_meshes)
// 5: the segmentation and vertex losses (pcnn_seg_loss, pcnn_cross_entropy, pcnn_vertex_loss,
//    pcnn_vertex_loss_compact and their workspace queries)
// 6: the backward of the class-compact vertex_pred layer (pcnn_vertex_pred_compact_bwd and its two queries)
// 7: the upscore layers (pcnn_upscore_fwd, pcnn_upscore_bwd, pcnn_upscore_compact_fwd, pcnn_upscore_compact_bwd
//    and the two workspace queries)
extern "C" int pcnn_abi_version(void) { return 8; }

extern "C" const char* pcnn_strerror(int code) {
  switch (code) {
    case PCNN_OK: return "ok";
    case PCNN_EINVAL: return "invalid argument";
    case PCNN_EHIP: return "HIP runtime error";
    case PCNN_ECAPACITY: return "workspace or output capacity too small";
    default: return "unknown error";
  }
}

namespace pcnn {
thread_local hipEvent_t t_done_event = nullptr;
}

// The next op called on this thread records `event` (a created hipEvent_t)
// when its last kernel completes; see pcnn_common.h launch_last.
extern "C" int pcnn_set_completion_event(void* event) {
  pcnn::t_done_event = (hipEvent_t)event;
  return PCNN_OK;
}

// 1 if the event set by pcnn_set_completion_event was not taken by an op's
// last launch (the op has no completion hook on this path); clears it.
extern "C" int pcnn_completion_event_pending(void) {
  const int p = pcnn::t_done_event != nullptr;
  pcnn::t_done_event = nullptr;
  return p;
}
