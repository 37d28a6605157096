// klatt_consts.h -- the few constants that the kernels (klatt_device.h, klatt_lanepipe.h, klatt_plan.h) and the host-only planning of a
// set call (klatt_batchplan.h) share.  Plain C++: no HIP include, so a native test can hold the planning to account on any machine.
#pragma once

#include <stdint.h>

namespace klatt {

constexpr int kLanes = 64;

constexpr uint32_t FRAME_NULL = 1u;       // FrameMeta.flags
constexpr uint32_t UTT_NEEDS_NOISE = 1u;  // UttDesc.flags
constexpr uint32_t UTT_NO_NASAL = 2u;     // UttDesc.flags: caNP == 0 throughout, N0/NP finite and stable (klatt_lanepipe.h)
constexpr uint32_t UTT_TRACKED = 4u;      // UttDesc.flags: noisy, every parameter finite, tracks planned
constexpr uint32_t UTT_DIRECT = 8u;       // UttDesc.flags: noisy, every parameter finite and in the range of klatt_math.h, no tracks: direct stages (klatt_direct.h)
// UttDesc.flags bits 4..6: terms that are PRESENT somewhere in the utterance's frame list (FACT_* of the same name, OR-ed over the list).  A flat
// stage whose wavefront holds no live lane with the bit runs a body without the term (klatt_systolic.h; option "dead_terms").
constexpr uint32_t UTT_TURBULENCE = 16u;  // voiceTurbulenceAmplitude is not +0.0 in every frame
constexpr uint32_t UTT_ASPIRATION = 32u;  // aspirationAmplitude is not +0.0 in every frame
constexpr uint32_t UTT_PARALLEL1 = 64u;   // parallel resonator 1 contributes, or might not stay finite
constexpr uint32_t kUttPresent = UTT_TURBULENCE | UTT_ASPIRATION | UTT_PARALLEL1;
constexpr int kUttKindShift = 8;         // UttDesc.flags bits 8..31 of a tracked utterance: the entry kinds (klatt_tracks) whose values change after the first sample
                                          // of its first fade -- a kind outside the mask of every lane of a wavefront is loaded once and never again (flat stages)

// FrameFacts.flags (klatt_plan.h)
constexpr uint32_t FACT_NOISE = 1u;        // a noise gain is non-zero, or the parallel bank's coefficients may not be finite
constexpr uint32_t FACT_NONFINITE = 2u;    // some parameter is NaN or infinite
constexpr uint32_t FACT_NASAL = 4u;        // the nasal pair is coupled in, or could not be skipped safely
constexpr uint32_t FACT_UNBOUNDED = 8u;    // a frequency or bandwidth outside the range of klatt_math.h, or a negative bandwidth (the direct stages)
constexpr uint32_t FACT_TURBULENCE = UTT_TURBULENCE;   // parameter 3 is not bit-for-bit +0.0
constexpr uint32_t FACT_ASPIRATION = UTT_ASPIRATION;   // parameter 6 is not bit-for-bit +0.0
constexpr uint32_t FACT_PARALLEL1 = UTT_PARALLEL1;     // pa1 is non-zero, or parallel resonator 1's output may not be finite (klatt_plan.h, shape_flags)

// A second word of PRESENT terms, of its own (UttDesc.flags is full): per frame in FrameFacts.present2 (klatt_plan.h), OR-ed per list
// (classify_list, ListTable.present2) and handed per utterance to the flat launch alone (KernelArgs.present2).  Same rule as above: a flat
// stage whose wavefront holds no live lane with the bit runs a body without the term.
constexpr uint32_t UTT2_PARALLEL2 = 1u;    // parallel resonator k (bit k - 2, k = 2..6) contributes, or might not stay finite
constexpr uint32_t UTT2_PARALLEL3 = 2u;
constexpr uint32_t UTT2_PARALLEL4 = 4u;
constexpr uint32_t UTT2_PARALLEL5 = 8u;
constexpr uint32_t UTT2_PARALLEL6 = 16u;
constexpr uint32_t UTT2_NASAL = 32u;       // FACT_NASAL of some frame: the nasal pair is coupled in, or could not be skipped safely
constexpr uint32_t kUtt2Present = 63u;
constexpr uint32_t kUtt2Parallel234 = UTT2_PARALLEL2 | UTT2_PARALLEL3 | UTT2_PARALLEL4;
constexpr int kDead2Counts = 4;            // the flat stages' second set of counters (dead2_wave_counts, klatt_batchplan.h)

}  // namespace klatt
