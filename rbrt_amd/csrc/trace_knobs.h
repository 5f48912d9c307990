// trace_knobs.h — the defaults of the trace kernel's lab knobs, defined ONCE: the scene handle (api.cpp) initialises its
// knobs from them, and the PLAIN build of the trace kernel (megakernel.inl) has them as compile-time constants. A launch
// runs the PLAIN build only while every knob of its TraceParams equals its default here (kernels.hip
// trace_params_are_plain), so a changed default changes the kernel with it and cannot leave it behind.
#pragma once
#include <stdint.h>

namespace rbrt {

struct TraceKnobs {
    uint32_t y_low_water;        // RBRT_Y_LOW
    uint32_t y_high_water;       // RBRT_Y_HIGH
    uint32_t y_high_min_parked;  // RBRT_Y_HIGH_PARKED
    uint32_t leaf_round;         // RBRT_LEAF_ROUND
    uint32_t leaf_leaves;        // RBRT_LEAF_LEAVES
    uint32_t share_idle;         // RBRT_SHARE_IDLE (0: no shared traversals)
    uint32_t shade_rounds;       // RBRT_SHADE_ROUNDS (rounds while work items are left; unbounded afterwards)
    uint32_t shade_cont_min;     // RBRT_SHADE_CONT_MIN
};
constexpr TraceKnobs kDefaultKnobs = {28u, 28u, 16u, 6u, 16u, 4u, 1u, 8u};
// RBRT_WORK_STRIPES: chunks (of 64 work items) per stripe for a launch that has the GPU to itself; 0 = contiguous shards.
// (Chosen per launch -- api.cpp, work_stripes_overlap -- so it stays a run-time value in every build of the kernel.)
constexpr uint32_t kDefaultWorkStripes = 16u;

// the ranges include/rbrt_hip_debug.h states, and what a launch's parameters always satisfy (api.cpp raises y_high_water
// to y_low_water)
static_assert(kDefaultKnobs.y_low_water >= 1u && kDefaultKnobs.y_low_water <= 64u && kDefaultKnobs.y_high_water >= kDefaultKnobs.y_low_water &&
                  kDefaultKnobs.y_high_water <= 64u && kDefaultKnobs.y_high_min_parked >= 1u && kDefaultKnobs.y_high_min_parked <= 256u,
              "default water marks outside their lab range");
static_assert(kDefaultKnobs.leaf_round >= 1u && kDefaultKnobs.leaf_round <= 64u && kDefaultKnobs.leaf_leaves >= 1u && kDefaultKnobs.leaf_leaves <= 128u &&
                  kDefaultKnobs.share_idle <= 64u && kDefaultKnobs.shade_rounds >= 1u && kDefaultKnobs.shade_cont_min >= 1u &&
                  kDefaultKnobs.shade_cont_min <= 64u,
              "default leaf / share / shade knobs outside their lab range");
static_assert((kDefaultWorkStripes & (kDefaultWorkStripes - 1u)) == 0u, "work stripes: 0 or a power of two (the kernel shifts)");

}  // namespace rbrt
