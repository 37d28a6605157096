// klatt_source.h -- the glottal source of a set batch (speechPlayer_batch_exportSource, _epochCounts, _exportEpochs).
//
// What every synthesis kernel's source stage does with the frame of a sample (dsp_sample, klatt_device.h; reference
// src/speechWaveGenerator.cpp:46-60, :72-83) and throws away: the vibrato phase V, the pitch after vibrato hz, the glottal phase P
// and the samples on which P wraps.  With cur(t) the frame klatt_timeline.h defines for sample t, V(-1) = P(-1) = 0, C(-1) = 0:
//     V(t) = frac(vibratoSpeed(t) / sr + V(t-1))               vib(t) = sin(V(t) * 2 pi) * 0.06 * vibratoPitchOffset(t) + 1
//     hz(t) = voicePitch(t) * vib(t)                            x(t) = hz(t) / sr + P(t-1)        P(t) = frac(x(t))
//     epoch(t) = x(t) finite and |x(t)| >= 1                    C(t) = C(t-1) + epoch(t)
// with the same device functions on the same operands in the same order as dsp_sample: div_by(., sampleRateF, invSampleRate),
// frac_toward_zero, the device library's sin.  (dsp_sample keeps V where vibratoSpeed is zero instead of adding the zero quotient: the
// same value, up to the sign of a zero.)  Nothing here depends on the noise seed, the arithmetic mode, the layout or the planner.
//
//   klatt_source_walk     ONE WAVEFRONT per frame list, 64 consecutive samples per pass.  Three chains are serial along a list --
//                         voicePitch (one addition per hold sample, the state machine of klatt_timeline_pitch taken one sample at
//                         a time), V and P -- and everything else is not: the lanes evaluate, side by side, the closed-form fades
//                         of the five other parameters, voicePitch inside fades, both quotients by the sample rate, the sine, the
//                         wrap test and the output columns.  A pass is
//                             chain 1 (wave-uniform): the request and the pitch state of each of the 64 samples, left in its lane
//                             lanes: parameters, vibratoSpeed / sr
//                             chain 2: V, lane i's quotient broadcast by two v_readlane_b32
//                             lanes: sin, hz, hz / sr
//                             chain 3: x and P, the same way
//                             lanes: wrap test (one ballot: C and the epoch's place in the table), columns, stores
//                         so the sine, by far the longest dependent piece, is never inside a serial loop.
//                         WHAT = kSourceColumns: the six columns at the steps phase + j * hop, 48 bytes per (list, step);
//                         kSourceCount: the list's number of epochs; kSourceEpochs: its epoch table, 32 bytes per epoch.
//   klatt_source_lanes    the same walk with ONE LANE per list, for batches of thousands of distinct lists (option "source_lane_lists").
//   klatt_source_dense    [row][step][column] of the chosen utterances from the step table, in the manner of klatt_timeline_dense.
//   klatt_source_deal     [row][epoch][4] of the chosen utterances from the lists' epoch tables, `pad` past a row's count.
// The request table (klatt_timeline_requests) and the fade rules (timeline_side, fade_value) are klatt_timeline.h's.  Built with
// -ffp-contract=off like the rest of the unit: every multiply and add below is rounded on its own.
#pragma once

#include <stdint.h>

#include "klatt_timeline.h"

namespace klatt {

constexpr int kSourceF0 = 0, kSourcePhase = 1, kSourceVibratoPhase = 2, kSourceCycle = 3, kSourceOpen = 4, kSourceWave = 5, kSourceCols = 6;
constexpr int kEpochCols = 4;                // sample, instant, f0, gain
constexpr int kSourceColumns = 0, kSourceCount = 1, kSourceEpochs = 2;      // what a walk leaves behind

struct SourceList {          // 40 B per list a walk takes
    long long frame0;
    long long nFrames;
    long long length;        // L
    long long out;           // kSourceEpochs: the list's first entry in the epoch table
    long long cap;           // ... and its number of entries (the count of the counting walk)
};
struct EpochRow {            // 16 B per output row of klatt_source_deal
    long long src;           // first entry of the row's list in the epoch table
    long long count;
};

__device__ __forceinline__ double source_broadcast(double v, int i)      // lane i's v in every lane (i wave-uniform)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), i);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Chain 1: voicePitch as klatt_timeline_pitch keeps it, taken one sample at a time.  pitch is curFrame.voicePitch after the sample,
// oldVp / newVp the two sides of the running fade (whose samples 1 .. F - 1 are the closed form fade_value(oldVp, newVp, c / F): the
// caller's business), k the request in effect and S its first sample.
struct SourcePitch {
    double pitch = 0.0, oldVp = 0.0, newVp = 0.0, inc = 0.0;
    long long k = -1, S = 0, next = 0, F = 0;
    bool oldNull = true, curNull = true;
};
__device__ __forceinline__ void source_pitch_step(SourcePitch& s, long long t, const double* __restrict__ frames, const FrameMeta* __restrict__ meta,
                                                  long long frame0)
{
    if (t == s.next) {                                                     // a dequeue: the frame of the sample before stays
        ++s.k;
        const FrameMeta m = meta[frame0 + s.k];
        s.S = t; s.F = m.fadeSamples; s.next = t + timeline_span(m);
        s.curNull = (m.flags & FRAME_NULL) != 0;
        double v = s.pitch, inc = 0.0;                                     // a NULL request: reference src/frame.cpp:62-63
        if (!s.curNull) {
            v = frames[(frame0 + s.k) * kNumParams];
            inc = (frames[(frame0 + s.k) * kNumParams + kNumParams - 1] - v) / (double)m.minSamples;      // :98
        }
        s.oldVp = !s.curNull && s.oldNull ? v : s.oldVp;                   // :65
        s.inc = inc;
        s.newVp = v + inc * (double)m.fadeSamples;                         // :71
    } else {
        const long long c = t - s.S;
        if (c == s.F) s.pitch = fade_value(s.oldVp, s.newVp, 1.0);         // the fade's last sample
        else if (c == s.F + 1) { s.oldVp = s.newVp; s.oldNull = s.curNull; }      // :44-47, the frame stays
        else if (c > s.F + 1) { s.pitch += s.inc; s.oldVp = s.pitch; }     // :77-78, one addition per hold sample
    }
}

template <int WHAT>
__global__ void __launch_bounds__(64) klatt_source_walk(const double* __restrict__ frames, const FrameMeta* __restrict__ meta,
                                                        const TimelineReq* __restrict__ req, const SourceList* __restrict__ lists,
                                                        double sampleRateF, double invSampleRate, long long hop, long long phase,
                                                        long long tableStride, double* __restrict__ table, long long* __restrict__ counts,
                                                        double* __restrict__ epochs)
{
    const SourceList list = lists[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const long long L = list.length;
    const TimelineReq* __restrict__ rq = req + list.frame0;
    SourcePitch ps;                         // chain 1
    double V = 0.0, P = 0.0;                // chains 2 and 3
    long long C = 0;
    long long nextStep = phase, jNext = 0;  // kSourceColumns: the first step not yet stored
    for (long long t0 = 0; t0 < L; t0 += 64) {
        const int n = L - t0 < 64 ? (int)(L - t0) : 64;
        const long long t = t0 + lane;
        const bool live = lane < n;
        double myPitch = 0.0, myOld = 0.0, myNew = 0.0;
        long long myK = 0;
        for (int i = 0; i < n; ++i) {
            source_pitch_step(ps, t0 + i, frames, meta, list.frame0);
            if (lane == i) { myPitch = ps.pitch; myOld = ps.oldVp; myNew = ps.newVp; myK = ps.k; }
        }
        // the lanes: the frame of sample t
        double vibDepth = 0.0, vibSpeed = 0.0, openQ = 0.0, voiceAmp = 0.0, preGain = 0.0;
        if (live) {
            const TimelineReq R = rq[myK];
            const long long c = t - R.first;
            if (c >= 1 && c <= (long long)R.fade) myPitch = fade_value(myOld, myNew, (double)c / (double)R.fade);
            if (c > 0 || myK > 0) {                                            // (sample 0 sees the zeroed frame of a fresh handle)
                const TimelineReq E = c == 0 ? rq[myK - 1] : R;
                const double ratio = c >= 1 && c <= (long long)R.fade ? (double)c / (double)R.fade : 1.0;
                const bool g0 = E.flags & 1u, g1 = E.flags & 2u;
                vibDepth = fade_value(timeline_side(frames, E.from, g0, 1), timeline_side(frames, E.to, g1, 1), ratio);
                vibSpeed = fade_value(timeline_side(frames, E.from, g0, 2), timeline_side(frames, E.to, g1, 2), ratio);
                if (WHAT == kSourceColumns) openQ = fade_value(timeline_side(frames, E.from, g0, 4), timeline_side(frames, E.to, g1, 4), ratio);
                if (WHAT != kSourceCount) voiceAmp = fade_value(timeline_side(frames, E.from, g0, 5), timeline_side(frames, E.to, g1, 5), ratio);
                if (WHAT == kSourceEpochs)
                    preGain = fade_value(timeline_side(frames, E.from, g0, kPreFormantGain), timeline_side(frames, E.to, g1, kPreFormantGain), ratio);
            }
        }
        // chain 2
        const double vq = div_by(vibSpeed, sampleRateF, invSampleRate);
        double myV = V;
        if (__ballot(live && vq != 0.0)) {                                     // (all quotients zero: V stays, frac(0 + V) = V)
            for (int i = 0; i < n; ++i) {
                V = frac_toward_zero(source_broadcast(vq, i) + V);
                if (lane == i) myV = V;
            }
        }
        const double vib = (sin(myV * 6.283185307179586) * 0.06 * vibDepth) + 1.0;
        const double hz = myPitch * vib;
        const double pq = div_by(hz, sampleRateF, invSampleRate);
        // chain 3
        double x = 0.0;
        for (int i = 0; i < n; ++i) {
            const double xi = source_broadcast(pq, i) + P;
            P = frac_toward_zero(xi);
            if (lane == i) x = xi;
        }
        const double myP = frac_toward_zero(x);
        const double ax = __builtin_fabs(x);
        const bool epoch = live && ax >= 1.0 && ax < __builtin_inf();
        const unsigned long long wraps = __ballot(epoch);
        const long long before = C + __popcll(wraps & ((1ull << lane) - 1ull));
        C += __popcll(wraps);
        if (WHAT == kSourceColumns) {
            const long long off = nextStep - t0;                               // >= 0
            if (off < 64) {
                const int o = (int)off, h = hop < 64 ? (int)hop : 64, d = lane - o;
                if (live && d >= 0 && d % h == 0) {
                    double* __restrict__ row = table + ((long long)blockIdx.x * tableStride + jNext + d / h) * kSourceCols;
                    const double cyc = (double)(before + (epoch ? 1 : 0));
                    *reinterpret_cast<double2*>(row) = make_double2(hz, myP);
                    *reinterpret_cast<double2*>(row + 2) = make_double2(myV, cyc);
                    *reinterpret_cast<double2*>(row + 4) = make_double2(myP >= openQ ? 1.0 : 0.0, ((myP * 2.0) - 1.0) * voiceAmp);
                }
                const long long cnt = (63 - o) / h + 1;                        // the steps of this pass (those past L are not stored)
                nextStep += cnt * hop; jNext += cnt;
            }
        }
        if (WHAT == kSourceEpochs) {
            if (epoch && before < list.cap) {
                double* __restrict__ row = epochs + (list.out + before) * kEpochCols;
                *reinterpret_cast<double2*>(row) = make_double2((double)t, (double)t - myP / (hz / sampleRateF));
                *reinterpret_cast<double2*>(row + 2) = make_double2(hz, voiceAmp * preGain);
            }
        }
    }
    if (WHAT == kSourceCount && lane == 0) counts[blockIdx.x] = C;
}

// The same walk with ONE LANE per frame list, for batches of thousands of distinct lists, where a wavefront per list spends its 64
// lanes on chains that use one: every lane carries its own three chains through its own list, one sample per iteration.  The five
// closed-form parameters are kept in registers: they move on the fade's samples 1 .. F alone -- the dequeue sample repeats the frame
// before, and a hold repeats fade_value(from, to, 1.0), the value of the fade's last sample (c / F = 1 exactly) -- so the frames are
// read once per request.  Same device functions, same operands, same order: the bits of klatt_source_walk.
template <int WHAT>
__global__ void __launch_bounds__(64) klatt_source_lanes(const double* __restrict__ frames, const FrameMeta* __restrict__ meta,
                                                         const TimelineReq* __restrict__ req, const SourceList* __restrict__ lists, long long nLists,
                                                         double sampleRateF, double invSampleRate, long long hop, long long phase,
                                                         long long tableStride, double* __restrict__ table, long long* __restrict__ counts,
                                                         double* __restrict__ epochs)
{
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nLists) return;
    const SourceList list = lists[l];
    const long long L = list.length;
    SourcePitch ps;
    constexpr int kCols[5] = {1, 2, 4, 5, kPreFormantGain};               // vibratoPitchOffset, vibratoSpeed, glottalOpenQuotient, voiceAmplitude
    double from[5], to[5], cur[5] = {0.0, 0.0, 0.0, 0.0, 0.0};            // (sample 0 sees the zeroed frame of a fresh handle)
    double V = 0.0, P = 0.0, fadeDiv = 1.0;
    long long C = 0, nextStep = phase, j = 0, k = -1;
    for (long long t = 0; t < L; ++t) {
        source_pitch_step(ps, t, frames, meta, list.frame0);
        if (ps.k != k) {                                                   // the dequeue sample: the request's two sides
            k = ps.k;
            const TimelineReq R = req[list.frame0 + k];
            fadeDiv = (double)R.fade;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                from[q] = timeline_side(frames, R.from, R.flags & 1u, kCols[q]);
                to[q] = timeline_side(frames, R.to, R.flags & 2u, kCols[q]);
            }
        }
        const long long c = t - ps.S;
        double pitch = ps.pitch;
        if (c >= 1 && c <= ps.F) {
            const double ratio = (double)c / fadeDiv;
            pitch = fade_value(ps.oldVp, ps.newVp, ratio);
#pragma unroll
            for (int q = 0; q < 5; ++q) cur[q] = fade_value(from[q], to[q], ratio);
        }
        V = frac_toward_zero(div_by(cur[1], sampleRateF, invSampleRate) + V);
        const double vib = (sin(V * 6.283185307179586) * 0.06 * cur[0]) + 1.0;
        const double hz = pitch * vib;
        const double x = div_by(hz, sampleRateF, invSampleRate) + P;
        P = frac_toward_zero(x);
        const double ax = __builtin_fabs(x);
        const bool epoch = ax >= 1.0 && ax < __builtin_inf();
        if (WHAT == kSourceEpochs && epoch && C < list.cap) {
            double* __restrict__ row = epochs + (list.out + C) * kEpochCols;
            *reinterpret_cast<double2*>(row) = make_double2((double)t, (double)t - P / (hz / sampleRateF));
            *reinterpret_cast<double2*>(row + 2) = make_double2(hz, cur[3] * cur[4]);
        }
        C += epoch ? 1 : 0;
        if (WHAT == kSourceColumns && t == nextStep) {
            double* __restrict__ row = table + (l * tableStride + j) * kSourceCols;
            *reinterpret_cast<double2*>(row) = make_double2(hz, P);
            *reinterpret_cast<double2*>(row + 2) = make_double2(V, (double)C);
            *reinterpret_cast<double2*>(row + 4) = make_double2(P >= cur[2] ? 1.0 : 0.0, ((P * 2.0) - 1.0) * cur[3]);
            ++j; nextStep += hop;
        }
    }
    if (WHAT == kSourceCount) counts[l] = C;
}

// Element e of the output is (row, step, column) as in klatt_timeline_dense; a lane owns 16 bytes.
template <bool F32>
__global__ void __launch_bounds__(256) klatt_source_dense(const double* __restrict__ table, long long tableStride, const TimelineRow* __restrict__ rows,
                                                          const long long* __restrict__ stepStart, const long long* __restrict__ chunkRow,
                                                          long long nRows, long long rowStride, const int* __restrict__ cols, int nCols,
                                                          void* __restrict__ outp, long long total, int vecStore)
{
    constexpr int EL = F32 ? 4 : 2;
    const long long nLane = (total + EL - 1) / EL;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nLane; t += stride) {
        const long long e0 = t * EL;
        long long g, r, j;
        int q;
        dense_locate(e0, nCols, rowStride, stepStart, chunkRow, g, q, r, j);
        TimelineRow row = rows[r];
        double v[EL];
#pragma unroll
        for (int i = 0; i < EL; ++i) {
            double x = 0.0;
            if (e0 + i < total) {
                if (rowStride == 0) while (j >= row.steps && r + 1 < nRows) { ++r; j = 0; row = rows[r]; }
                if (j < row.steps) x = table[((long long)row.slot * tableStride + j) * kSourceCols + cols[q]];
                if (++q == nCols) {
                    q = 0; ++j;
                    if (rowStride > 0 && j == rowStride && r + 1 < nRows) { ++r; j = 0; row = rows[r]; }
                }
            }
            v[i] = x;
        }
        store16<typename std::conditional<F32, float, double>::type>(outp, e0, total, vecStore, v);
    }
}

// One lane per entry of the output: entry g is (row, epoch) = (g / rowStride, the rest) or, packed, by bisection over the rows' starts.
__global__ void __launch_bounds__(256) klatt_source_deal(const double* __restrict__ epochs, const EpochRow* __restrict__ rows,
                                                         const long long* __restrict__ start, long long nRows, long long rowStride, double pad,
                                                         double* __restrict__ out, long long entries, int vecStore)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < entries; g += stride) {
        long long r, j;
        if (rowStride > 0) { r = g / rowStride; j = g - r * rowStride; }
        else packed_locate(g, start, nRows, r, j);
        const EpochRow row = rows[r];
        double* __restrict__ o = out + g * kEpochCols;
        double2 a = make_double2(pad, pad), b = a;
        if (j < row.count) {                                           // (the table is the engine's own: 16-byte aligned)
            const double2* __restrict__ s = reinterpret_cast<const double2*>(epochs + (row.src + j) * kEpochCols);
            a = s[0]; b = s[1];
        }
        if (vecStore) { reinterpret_cast<double2*>(o)[0] = a; reinterpret_cast<double2*>(o)[1] = b; }
        else { o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y; }
    }
}

}  // namespace klatt
