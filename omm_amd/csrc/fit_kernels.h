// fit_kernels.h -- ommxProfileMicromapLevels: what every block of a device-resident result would keep at every coarser level (fit_kernels.hip; the
// definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool and the argument checks; the two calls below are the
// phases between which the host has to size a block of memory.  ommxFitMicromap reads the same arrays back as the table of fit_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "fit_plan.h"

namespace ommx {

struct ProfileArgs {
    ommCpuBakeResultDesc result;        // host struct, arrays in device memory; indexFormat already checked
    const float* weights;               // [indexCount] device memory, or null: every primitive counts 1
    // device memory; null: the array lives in the call's scratch (profile_arrays says where)
    uint32_t *known, *opaque;           // [descArrayCount][kFitLevels]
    uint32_t* refs;                     // [descArrayCount]
    unsigned long long* blockWeights;   // [descArrayCount]
    uint32_t* shape;                    // [descArrayCount] the words of fit_plan.h: in the scratch when wantShape, otherwise not written
    bool wantShape;
};
struct ProfilePlan {                    // after the index buffer has been read
    uint64_t units;                     // work units of the counting pass: one byte of scratch each (the state of the unit's root)
    uint32_t deepBlocks;                // blocks above level 8: a second pass finishes them
    uint32_t skipped, referenced;
    int32_t weightExponent;
};

size_t profile_head_bytes(const ProfileArgs& a);
ProfileArgs profile_arrays(const ProfileArgs& a, void* head);   // a with the arrays that live in the scratch pointed there
// each: every launch on `stream`, the answer copied to the host, the stream synchronised.  indexCount must be > 0.
hipError_t profile_plan(const ProfileArgs& a, void* head, ProfilePlan* out, hipStream_t stream);
hipError_t profile_count_blocks(const ProfileArgs& a, void* head, void* roots, const ProfilePlan& plan, hipStream_t stream);

} // namespace ommx
