// klatt_layout.h -- the layouts that the host's track planner (klatt_trackplan.h), the live handles' host half (klatt_live.h) and the
// kernels (klatt_device.h, klatt_tracks.h, klatt_direct.h, klatt_plan.h) share: a frame's meta word, an utterance's descriptor and
// result, the track block, a direct job.  Plain C++: no HIP include, so a native test can hold the host code to account on any
// machine.  klatt_device.h includes it; the kernels see what they always saw.
#pragma once

#include <stdint.h>

#include "klatt_consts.h"

// functions of both sides: under hipcc exactly the attributes they always had, nothing for a host compiler
#if defined(__HIPCC__)
#define KLATT_LAYOUT_HD __host__ __device__
#else
#define KLATT_LAYOUT_HD
#endif

namespace klatt {

constexpr int kNumParams = 47;
constexpr int kNumRes = 14;

struct FrameMeta {           // 16 B per frame; with the 376-B parameter vector: 392 B/frame read
    uint32_t minSamples;
    uint32_t fadeSamples;    // already clamped to >= 1 (reference src/speechPlayer.cpp:36)
    int32_t userIndex;
    uint32_t flags;
};

struct UttDesc {             // 32 B per utterance
    long long frameStart;    // first frame (index into frames / meta)
    long long outStart;      // sample offset in the PCM pool, multiple of kTile
    uint32_t nFrames;
    uint32_t seed;
    uint32_t flags;          // UTT_NEEDS_NOISE: some frame has a non-zero (or non-finite) noise gain
    uint32_t length;         // samples this utterance produces (closed form, host-computed)
};

struct UttResult {           // written by the kernel
    uint32_t produced;       // samples written by this launch
    uint32_t framesTaken;    // frames dequeued by this launch
    int32_t lastIndex;
    uint32_t drained;        // 1: the queue ran dry (short count)
};

// ---- tracks (klatt_tracks.h) ---------------------------------------------------------------------------------
// A resonator's coefficients are a pure function of (f, bw) (reference src/speechWaveGenerator.cpp:112-127), and during a
// fade every parameter is a pure function of the fade's two end frames and the sample counter (reference src/frame.cpp:48-53):
// what the filter stages need on a fade sample does not depend on the signal.  The tracked kernels therefore take it from a
// TRACK -- evaluated densely (lanes = entries) by klatt_tracks before the synthesis launch -- instead of interpolating and
// evaluating exp/cos inside the sample recurrence.  A track is an array of 16-byte entries, kTrackEntries kinds of them:
//   0..13   resonator r (N0, NP, c6..c1, p1..p6): (b, c); a = 1 - b - c, except for the anti-resonator N0, whose a is a
//           second entry (a, -) right after its (b, c)
//   14..19  the interpolated gains of the filter stages, in pairs: (caNP, -) | (pa5, pa6) (parallelBypass, outputGain) |
//           (fricationAmplitude, preFormantGain) (pa1, pa2) (pa3, pa4)          -- S1 | final stage | parallel stage
//   20..23  the source stage's parameters: (vibratoPitchOffset, vibratoSpeed) (voiceTurbulenceAmplitude, glottalOpenQuotient)
//           (voiceAmplitude, aspirationAmplitude) (preFormantGain, -)           -- S0 (the pitch itself glides: not in a track)
// On fade sample 1 everything is re-evaluated (see fade_update in klatt_device.h): every kind has an entry for it, kTrackFirst entries (N0
// takes two).  Fade samples 2..F change only the kinds that MOVE in the fade (mask).  A fade's track is four PARTS, one per flat
// stage (S0: kinds 0, 1, 14, 20..23 | S1: 2..7 | final stage: 12, 13, 15, 16 | parallel stage: 8..11, 17..19 -- KLATT_FLAT_LAYOUT in klatt_device.h), so that what a
// stage streams through is contiguous and no cache line is shared by two stages -- which work 16 to 32 samples apart: with the
// kinds of all stages interleaved in one row a line was fetched once per stage, 34 GB from HBM per launch of a batch with 445 MB
// of tracks, for 22 GB of rows.  Layout of a part:
//   header   the stage's kinds that do NOT move, ascending: their value of fade sample 1 (which is their value on every later sample)
//   matrix   F rows of the stage's kinds that move, ascending (N0 takes two); row j holds fade sample j + 1
// so a moving kind's entries are one stride (the part's moving entries) apart from the first fade sample on, and a kind that
// does not move has ONE entry: a stage points at it with stride 0.  kTrackFirst + (F - 1) * nSlots entries in all.
// Fades with bitwise equal end values of all the parameters involved and the same length share one track (host, plan_tracks).
constexpr int kTrackEntries = 24;
constexpr int kTrackFirst = kTrackEntries + 1;   // entries of a fade's first sample (N0 takes two)
constexpr int kShapeValues = 45;                 // a SHAPE: the parameter values a track depends on at one end of the fade
constexpr int kShapeStride = 46;
// where the values of a shape come from in a frame: (f, bw) of resonator r at 2r, 2r + 1; then the gains
KLATT_LAYOUT_HD constexpr int shape_param(int i)
{
    constexpr int kF[14] = {13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30};
    constexpr int kB[14] = {21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36};
    constexpr int kG[17] = {23, 41, 42, 43, 45, 24, 44, 37, 38, 39, 40, 1, 2, 3, 4, 5, 6};
    return i < 28 ? ((i & 1) ? kB[i >> 1] : kF[i >> 1]) : kG[i - 28];
}
constexpr int kShapePreGain = 28 + 6;            // preFormantGain (parameter 44): silence gates it (reference src/frame.cpp:61,66)
// the two shape values of gain entry e (14..19); -1: none
KLATT_LAYOUT_HD constexpr int entry_value(int e, int half)
{
    constexpr int kV[10][2] = {{28, -1}, {29, 30}, {31, 32}, {33, 34}, {35, 36}, {37, 38}, {39, 40}, {41, 42}, {43, 44}, {34, -1}};
    return kV[e - 14][half];
}
struct TrackRef {            // per frame on the host (plan_tracks); the stages read it as a FlatRef
    unsigned long long off;  // first entry of the fade's track
    uint32_t mask;           // entry kinds that move in the fade (bit e)
    uint32_t nSlots;         // entries per fade sample after the first: popcount(mask) + (mask & 1)
};
struct FlatRef {             // 16 B per frame: what a flat stage needs when the frame's fade starts, in one load (host: setUtterances)
    uint32_t off;            // first entry of the fade's track (tracks hold fewer than 2^32 entries: 64 GB)
    uint32_t mask;           // entry kinds that move in the fade
    uint32_t fadeSamples;
    uint32_t span;           // samples from this frame's dequeue to the next frame's: max(minSamples, fadeSamples + 1) + 1
};
struct SourceRef {           // 32 B per frame: what the flat source stage needs when the frame is dequeued, in two loads (host: setUtterances)
    double pitch;            // voicePitch (parameter 0)
    double pitchInc;         // (endVoicePitch - voicePitch) / minSamples     (reference src/frame.cpp:98; the host's division is the device's: IEEE)
    double invFade;          // 1 / fadeSamples
    int32_t userIndex;
    uint32_t flags;          // FRAME_NULL
};
struct TrackJob {            // one distinct track, read by klatt_tracks
    unsigned long long off;
    uint32_t fromShape, toShape;    // the fade's end points (index into TrackArgs.shapes)
    uint32_t fadeSamples;
    uint32_t mask;
};
KLATT_LAYOUT_HD inline uint32_t track_slots(uint32_t mask) { return (uint32_t)__builtin_popcount(mask) + (mask & 1u); }

// ---- direct stages (klatt_direct.h) ---------------------------------------------------------------------------
struct DirectJob {           // host -> klatt_seeds: the end points of one frame's fade (reference src/frame.cpp:55-72, walked on the host)
    uint32_t frame;          // the frame (durations: meta[frame])
    uint32_t from, to;       // the frames whose values the fade starts from / ends on; kNoFrame: all zero (a fresh handle)
    uint32_t flags;          // bit 0: the start's preFormantGain is gated off, bit 1: the end's (silence, reference src/frame.cpp:61,66)
};
constexpr uint32_t kNoFrame = 0xFFFFFFFFu;

}  // namespace klatt
