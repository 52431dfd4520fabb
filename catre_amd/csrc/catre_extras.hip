// catre_extras.hip - the unit of libcatre_hip.so around the refine path: train-time augmentation and init noise, point-cloud
// preparation (per image and per frame batch), NOCS alignment, tracking, trimmed ICP, the splat render, the mesh rasteriser, the
// BOP pose errors,
// the training loss and the device evaluator, each as a kernel header and its C ABI beside it.
#include <algorithm>
#include <cstring>

#include "catre_aug.h"
#include "catre_pcl.h"
#include "catre_pclf.h"
#include "catre_align.h"
#include "catre_track.h"
#include "catre_icp.h"
#include "catre_render.h"
#include "catre_mesh.h"
#include "catre_bop.h"
#include "catre_loss.h"
#include "catre_eval.h"

#include "catre_host.h"
using namespace catre_host;

extern "C" {
#include "catre_aug_api.inc"
#include "catre_pcl_api.inc"
#include "catre_pclf_api.inc"
#include "catre_align_api.inc"
#include "catre_track_api.inc"
#include "catre_icp_api.inc"
#include "catre_zbuf_api.inc"
#include "catre_render_api.inc"
#include "catre_mesh_api.inc"
#include "catre_bop_api.inc"
#include "catre_loss_api.inc"
#include "catre_eval_api.inc"
}  // extern "C"
