// The per-slot sampler step (sampler.hip): the PLMS / DDIM step of launch_sampler_step for up to SDMI_SAMPLER_MAX_SLOTS independent
// latents in one launch.  The descriptors are include/sdmi.h's; the launcher adds the host scalars of launch_sampler_step to each.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdmi.h"

namespace sdmi {
int launch_sampler_step_rows(const sdmi_sampler_slot* slots, int n_slots, int64_t n, hipStream_t s);
// ... and for slots of two kinds, that step or one evaluation of a DPM-Solver plan with its update, the next timestep written as fp32
int launch_sampler_plan_rows(const sdmi_sampler_plan_slot* slots, int n_slots, int64_t n, hipStream_t s);
}  // namespace sdmi
