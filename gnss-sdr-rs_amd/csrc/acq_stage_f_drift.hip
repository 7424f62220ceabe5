// acq_stage_f_drift.hip — stage F of a handle with code-drift compensation (gm_acq_set_code_drift): acq_stage_f_variants.h's three
// kernels with DriftLoad, instantiated for every plan they can run on.
// The three families share one source and take a unit each: in one unit they were the longest job of the build.  None of them shares
// a unit with the K = 1 kernels, whose sources and code objects stay exactly as they are.
#include "acq_stage_f_variants.h"

namespace gm {

template StageFLaunch find_stage_f<DriftLoad>(int, int);

}  // namespace gm
