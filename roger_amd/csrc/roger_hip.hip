// roger_hip.hip -- kernels and C ABI of the MI355X-native SVAT backend (see include/roger_hip.h).
//
// Kernel inventory (one thread = one soil column, 256-thread workgroups = 4 wavefronts):
//   k_pred1        start-of-step predicates over swe/swe_top, grid-stride, one word per workgroup
//   k_agg          1 workgroup: [user hooks] + OR of the workgroup words + forcing predicates,
//                  step-class flags, aggregates of the shared forcing series (numpy summation order)
//   k_select       prec/ta selection per column, event + infiltration predicates, one word per workgroup
//   k_scalars      1 workgroup: OR of the words, time-step bookkeeping (dt, event ids, itt, time),
//                  StepCtx for the step
//   k_step<M>      THE hot kernel: whole SVAT step per column, state read once / written once
//   k_reduce       only for multi-GPU runs: materialises a predicate word for the all-reduce
// plus one kernel per routine for the per-routine entry points and the setup-time kernels.
// All per-column kernels are HBM-bound streaming kernels (no data reuse, no LDS tiling, no
// MFMA); k_step moves ~2 KB per column (2.8 KB by the reference's variable read/write sets).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the entry points are resolved with dlsym on first use (rccl_api)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rh_host.h"
#include "rh_physics.h"
#include "rh_sets.inc"
#include "roger_hip.h"

#include "rh_dev_state.h"
#include "rh_control.h"
#include "rh_zonal.h"
#include "rh_step.h"
#include "rh_routing.h"
#include "rh_scores.h"   // (last: the kernels in front of it keep their places in the code object)
#include "rh_events.h"   // (behind it, for the same reason)
#include "rh_durations.h"   // (and behind that)
#include "rh_bands.h"   // (and behind that)

// The host side, one file per concern.  The entry points get their C linkage from their declarations in roger_hip.h.
#include "rh_host_kernels.h"
#include "rh_context.h"
#include "rh_rccl.h"
#include "rh_observers.h"
#include "rh_setup.h"
#include "rh_forcing.h"
#include "rh_routing_host.h"
#include "rh_stepping.h"
#include "rh_tools.h"
