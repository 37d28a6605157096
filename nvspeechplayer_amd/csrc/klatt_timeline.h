// klatt_timeline.h -- the timeline of a set batch and its per-sample parameter tracks (speechPlayer_batch_exportTracks).
//
// What the synthesis kernels interpolate and throw away -- the frame getCurrentFrame() hands the wave generator on every sample
// (reference src/frame.cpp:41-80, :121-126) -- evaluated for chosen utterances, columns and sample positions, straight from the frames,
// the 16-byte meta words and the list table that any set call leaves resident.  Nothing here depends on the arithmetic mode, the
// layout, the planner's choices or on whether the batch has been synthesised.
//
// Request k of a list is dequeued on sample S_k = sum_{i<k} (max(M_i, F_i + 1) + 1) (on that sample, and on sample 0, the frame is the one
// of the sample before); c = t - S_k counts the samples since.  With (o, t) the old and the new side of the fade after the NULL rules of
// frame.cpp:59-67 (walk_fade_ends: a source frame and a gate on preFormantGain for either side) and f(o, t, r) = isnan(t) ? o : o + (t - o) * r
// (src/utils.h:20-23), every parameter but voicePitch is
//     c = 0: f(o_{k-1}, t_{k-1}, 1.0) (zero for k = 0)     1 <= c <= F_k: f(o_k, t_k, c / F_k)     beyond: f(o_k, t_k, 1.0)
// -- the hold keeps the value of the fade's LAST sample, not the target.  voicePitch alone is sequential: both sides of its fade are
// what the previous requests left behind (:62, :71, :78), and a hold adds the request's increment once per sample (:77).
//
//   klatt_timeline_requests  one lane per frame list: 32 bytes per request (S_k, F_k, the two source frames and gates, the running
//                            index mark).  Once per set call, at the first export.
//   klatt_timeline_pitch     one lane per list a chosen utterance speaks, only when column 0 is asked for: carries voicePitch through
//                            fades and holds as the reference does -- one dependent f64 addition per hold sample -- and stores it at the
//                            step positions (8 bytes per (list, step)).
//   klatt_timeline_dense     the store-bound part, in the manner of pcm_export: consecutive lanes own consecutive 16 bytes of the
//                            [row][step][column] output; per step the request by bisection over the list's S_k, then the closed form,
//                            reading the two source frames from the batch's own frame buffer.
// The translation unit is built with -ffp-contract=off: o + (t - o) * r stays an add, a multiply and an add, and c / F_k is the
// correctly rounded f64 quotient, as in the reference.
#pragma once

#include <stdint.h>

#include <type_traits>

#include "klatt_device.h"
#include "klatt_tiles.h"

namespace klatt {

constexpr int kTrackMark = 47, kTrackFrame = 48, kTrackColumns = 49;
constexpr int kPreFormantGain = 44;          // the parameter silence gates off (reference src/frame.cpp:61,66)

struct TimelineReq {         // 32 B per frame (request)
    long long first;         // S_k: the sample the request is dequeued on
    uint32_t fade;           // F_k
    uint32_t from, to;       // the frames the fade starts from / ends on; kNoFrame: all zero (a fresh handle)
    uint32_t flags;          // bit 0: the start's preFormantGain is gated off, bit 1: the end's
    int32_t mark;            // what getLastIndex() answers once the request has been dequeued
    uint32_t pad;
};
static_assert(sizeof(TimelineReq) == 32, "TimelineReq layout");

struct TimelineList {        // a list klatt_timeline_pitch walks
    long long frame0;
    long long nFrames;
};
struct TimelineRow {         // 24 B per output row
    long long frame0;        // first frame of the row's list
    uint32_t nFrames;
    uint32_t slot;           // row of the pitch table that holds its list's voicePitch
    long long steps;         // ceil((L - phase) / hop), 0 when L <= phase
};
static_assert(sizeof(TimelineRow) == 24, "TimelineRow layout");

__host__ __device__ inline long long timeline_span(const FrameMeta& m)      // samples from a request's dequeue to the next one's
{
    const long long M = m.minSamples, F = m.fadeSamples;
    return (M > F + 1 ? M : F + 1) + 1;
}

__global__ void __launch_bounds__(256) klatt_timeline_requests(const FrameMeta* __restrict__ meta, const long long* __restrict__ listStart,
                                                               long long nLists, TimelineReq* __restrict__ req)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < nLists; l += stride) {
        long long S = 0;
        uint32_t prevReal = kNoFrame;
        bool prevNull = true;
        int32_t mark = -1;
        for (long long k = listStart[l]; k < listStart[l + 1]; ++k) {
            const FrameMeta m = meta[k];
            TimelineReq r;
            r.first = S; r.fade = m.fadeSamples; r.pad = 0;
            if (m.flags & FRAME_NULL) {
                r.from = prevReal; r.to = prevReal;
                r.flags = (prevNull ? 1u : 0u) | 2u;
                prevNull = true;
            } else {
                r.to = (uint32_t)k;
                r.from = prevNull ? (uint32_t)k : prevReal;
                r.flags = prevNull ? 1u : 0u;
                prevReal = (uint32_t)k;
                prevNull = false;
            }
            if (m.userIndex != -1) mark = m.userIndex;
            r.mark = mark;
            req[k] = r;
            S += timeline_span(m);
        }
    }
}

// voicePitch of one list at the samples phase + j * hop, into pitch[slot * pitchStride + j].  State as in the reference: P is
// curFrame.voicePitch, oldVp the old request's frame.voicePitch (the new request's adjusted value after a fade, the running value
// after a hold sample, the new frame's own value when the old request was silence).
__global__ void __launch_bounds__(64) klatt_timeline_pitch(const double* __restrict__ frames, const FrameMeta* __restrict__ meta,
                                                           const TimelineList* __restrict__ lists, long long nLists, long long hop, long long phase,
                                                           long long pitchStride, double* __restrict__ pitch)
{
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nLists) return;
    const TimelineList list = lists[l];
    double* __restrict__ out = pitch + l * pitchStride;
    double P = 0.0, oldVp = 0.0;
    bool oldNull = true;
    long long S = 0, next = phase, j = 0;
    for (long long k = list.frame0; k < list.frame0 + list.nFrames; ++k) {
        const FrameMeta m = meta[k];
        const long long F = m.fadeSamples, span = timeline_span(m);
        double inc, newVp;
        if (m.flags & FRAME_NULL) {
            newVp = P; inc = 0.0;                                          // :62-63
        } else {
            const double v = frames[k * kNumParams], e = frames[k * kNumParams + kNumParams - 1];
            inc = (e - v) / (double)m.minSamples;                          // :98 (infinite or NaN when minFrameDuration is 0)
            if (oldNull) oldVp = v;                                        // :65
            newVp = v;
        }
        newVp = newVp + inc * (double)m.fadeSamples;                       // :71
        const double fadeDiv = (double)m.fadeSamples;
        // the dequeue sample and the fade: a closed form of (oldVp, newVp), evaluated at the steps alone
        while (next <= S + F && next < S + span) {
            const long long c = next - S;
            out[j++] = c == 0 ? P : fade_value(oldVp, newVp, (double)c / fadeDiv);
            next += hop;
        }
        P = fade_value(oldVp, newVp, 1.0);                                 // the fade's last sample (c = F: the ratio is exactly 1)
        if (next == S + F + 1) { out[j++] = P; next += hop; }              // :44-47, the frame stays
        oldVp = newVp;
        oldNull = (m.flags & FRAME_NULL) != 0;
        for (long long c = F + 2; c < span; ++c) {                         // :77-78, one addition per hold sample
            P += inc;
            if (S + c == next) { out[j++] = P; next += hop; }
        }
        if (span > F + 2) oldVp = P;
        S += span;
    }
}

__device__ __forceinline__ double timeline_side(const double* __restrict__ frames, uint32_t src, bool gated, int col)
{
    if (src == kNoFrame || (gated && col == kPreFormantGain)) return 0.0;
    return frames[(long long)src * kNumParams + col];
}

// kTimelineChunkLog2, packed_locate and dense_locate -- the row of an output's entry -- are klatt_tiles.h's: the host compiles them too.

// A lane's 16 bytes: EL elements of T from element e0 of the output, one store where the output is aligned and the lane is whole.
template <typename T, typename V, int EL>
__device__ __forceinline__ void store16(void* __restrict__ outp, long long e0, long long total, int vecStore, const V (&v)[EL])
{
    static_assert(sizeof(T) * EL == 16, "a lane owns 16 bytes");
    struct alignas(16) Lane { T x[EL]; };
    T* o = static_cast<T*>(outp) + e0;
    if (vecStore && e0 + EL <= total) {
        Lane l;
#pragma unroll
        for (int i = 0; i < EL; ++i) l.x[i] = (T)v[i];
        *reinterpret_cast<Lane*>(o) = l;
    } else for (int i = 0; i < EL && e0 + i < total; ++i) o[i] = (T)v[i];
}

// A lane owns 16 bytes: 4 float32 or 2 float64 elements (dense_locate).
template <bool F32>
__global__ void __launch_bounds__(256) klatt_timeline_dense(const double* __restrict__ frames, const TimelineReq* __restrict__ req,
                                                            const TimelineRow* __restrict__ rows, const long long* __restrict__ stepStart,
                                                            const long long* __restrict__ chunkRow, long long nRows, long long rowStride,
                                                            const int* __restrict__ cols, int nCols, long long hop, long long phase,
                                                            const double* __restrict__ pitch, long long pitchStride,
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
        // the request of the step in hand, kept while the following elements stay inside it
        long long k = -1, kFirst = 0, kNext = 0;
        TimelineReq R, Rp;
        bool havePrev = false;
        double v[EL];
#pragma unroll
        for (int i = 0; i < EL; ++i) {
            double x = 0.0;
            if (e0 + i < total) {
                if (rowStride == 0) while (j >= row.steps && r + 1 < nRows) { ++r; j = 0; row = rows[r]; k = -1; }      // (rows without steps are stepped over)
                if (j < row.steps) {
                    const long long s = phase + j * hop;
                    if (k < 0 || s < kFirst || s >= kNext) {
                        long long lo = 0, hi = row.nFrames;             // the last request dequeued on or before s
                        const TimelineReq* __restrict__ rq = req + row.frame0;
                        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (rq[mid].first <= s) lo = mid; else hi = mid; }
                        k = lo; R = rq[k]; kFirst = R.first;
                        kNext = k + 1 < (long long)row.nFrames ? rq[k + 1].first : 0x7FFFFFFFFFFFFFFFll;
                        havePrev = false;
                    }
                    const int col = cols[q];
                    const long long c = s - kFirst;
                    if (col == kTrackMark) x = (double)R.mark;
                    else if (col == kTrackFrame) x = (double)k;
                    else if (col == 0) x = pitch[(long long)row.slot * pitchStride + j];
                    else if (c == 0) {
                        if (k > 0) {
                            if (!havePrev) { Rp = req[row.frame0 + k - 1]; havePrev = true; }
                            x = fade_value(timeline_side(frames, Rp.from, Rp.flags & 1u, col), timeline_side(frames, Rp.to, Rp.flags & 2u, col), 1.0);
                        }
                    } else {
                        const double ratio = c <= (long long)R.fade ? (double)c / (double)R.fade : 1.0;
                        x = fade_value(timeline_side(frames, R.from, R.flags & 1u, col), timeline_side(frames, R.to, R.flags & 2u, col), ratio);
                    }
                }
                // the next element: the next column, the next step, the next row
                if (++q == nCols) {
                    q = 0; ++j;
                    if (rowStride > 0 && j == rowStride && r + 1 < nRows) { ++r; j = 0; row = rows[r]; k = -1; }
                }
            }
            v[i] = x;
        }
        store16<typename std::conditional<F32, float, double>::type>(outp, e0, total, vecStore, v);
    }
}

}  // namespace klatt
