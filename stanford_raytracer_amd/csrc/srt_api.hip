// srt_api.hip -- C ABI (include/srt.h) of the MI355X-native many-ray Haselgrove integrator.
// Host side: model construction (device-resident tables), kernel launches, HIP-event timing.
// There is no CPU fallback: every entry point fails with SRT_EDEVICE when no GPU is usable.
//
// The library's one HIP translation unit.  Its body is the units below, one header per subsystem; each says at its top what it
// owns and includes what it uses, so the order here is only the order of the listing.  Dependencies run one way: core <- model
// <- the rest.  Where a unit calls another's extern "C" entry point, the declaration in include/srt.h is the dependency.
//
//   srt_api_core.hpp     errors, DevBuf, device selection and DeviceScope, struct srt_model, with_model, the shared macros
//   srt_api_model.hpp    fill_common / model_finish, destroy and trim, field options, getters; the Ngo, Ngo3d, simple3d,
//                        AT64ThCh and scattered constructors; the scattered model's scratch policy
//   srt_api_grid.hpp     modelnum 3: coefficient and node-table build, layouts, constructors; srt_build_grid; srt_dump_model
//   srt_api_points.hpp   the per-point calls: plasma parameters, dispersion, field-line foot, handedness, gradients, RK step
//   srt_api_sampler.hpp  srt_build_samples
//   srt_api_trace.hpp    trace_launch and the trace entry points, whole and in segments; srt_trace_batch; srt_trace_run_*
//   srt_api_rows.hpp     damping, row packing, the packed-row contract, crossings, approaches, binning
#include "srt_api_core.hpp"
#include "srt_api_model.hpp"
#include "srt_api_grid.hpp"
#include "srt_api_points.hpp"
#include "srt_api_sampler.hpp"
#include "srt_api_trace.hpp"
#include "srt_api_rows.hpp"
