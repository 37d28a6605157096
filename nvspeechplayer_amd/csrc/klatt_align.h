// klatt_align.h -- phoneme alignment of a batch set from IPA text (speechPlayer_batch_exportAlignment, speechPlayer_batch_exportUnits).
//
// The frame producer knows, for every frame it emits, which phoneme-table row it stands for, its stress and prosodic bits, whether it is
// an inserted pre-stop gap or post-stop aspiration, which text symbol it belongs to (its UNIT) and where that symbol sits in the caller's
// string: a 16-byte label per frame of a LIST (include/speechPlayer_batch.h, speechPlayer_frameLabel_t).  A set call with labels leaves
// them resident beside the frames, together with unitFirst[]: per list the first frame of every unit and, one past the last unit, the
// list's frame count (list l's entries start at listStart[l] + l: a list has at most as many units as frames).
//
// The timing half is klatt_timeline.h's: request k of a list takes effect on sample S_k (TimelineReq::first, built once per set call by
// klatt_timeline_requests), and the request in effect on sample t is the last one with S_k <= t -- the utterance's last sample (the +1 of
// the last request's span) belongs to the last request.  A label on sample t is a gather through that request.
//
//   klatt_align_dense   framewise labels, store-bound, in the manner of klatt_timeline_dense / pcm_export: consecutive lanes own
//                       consecutive 16 bytes of the [row][step][column] output (4 int32 or 2 int64 elements); per step the request by
//                       bisection over the list's S_k, kept while the lane's following elements stay inside it; the label, and for
//                       `position` / `remaining` the unit's first sample and the next unit's, read once per request.
//   klatt_align_units   the segment table: one lane per (row, unit) -- or per (row, frame) -- of the output, 7 int64 columns.
// Integers only: nothing here depends on the arithmetic mode or on -ffp-contract.
#pragma once

#include <stdint.h>

#include "klatt_timeline.h"

namespace klatt {

struct FrameLabel {          // speechPlayer_frameLabel_t
    int32_t phoneme;
    uint32_t flags;
    int32_t unit;
    int32_t textOffset;
};
static_assert(sizeof(FrameLabel) == 16, "FrameLabel layout");

constexpr int kAlignPhoneme = 0, kAlignStress = 1, kAlignFlags = 2, kAlignUnit = 3, kAlignTextOffset = 4, kAlignFrame = 5, kAlignPosition = 6,
              kAlignRemaining = 7, kAlignColumns = 8;
constexpr int kUnitColumns = 7;             // phoneme, flags, textOffset, firstSample, samples, firstStep, steps
constexpr uint32_t kLabelGap = 128u, kLabelPuff = 256u;

struct AlignRow {            // 40 B per output row
    long long frame0;        // first frame of the row's list
    long long unit0;         // where the list's unitFirst[] begins
    long long count;         // dense: ceil((L - phase) / hop), 0 when L <= phase; units: the row's entries (units or frames)
    uint32_t nFrames;
    uint32_t nUnits;
    uint32_t length;         // L: the utterance's samples
    uint32_t pad;
};
static_assert(sizeof(AlignRow) == 40, "AlignRow layout");

// the steps phase + j * hop below sample x
__host__ __device__ inline long long align_steps_below(long long x, long long hop, long long phase)
{
    return x > phase ? (x - phase + hop - 1) / hop : 0;
}

// Element e of the output is (row, step, column) as in klatt_timeline_dense: g = e / nCols the step's number in the output, the row
// g / rowStride (padded) or by bisection over stepStart within the chunk table's bounds (packed).  needSpan: a column among
// `position` / `remaining` is asked for (uniform over the launch).
template <bool I32>
__global__ void __launch_bounds__(256) klatt_align_dense(const TimelineReq* __restrict__ req, const FrameLabel* __restrict__ labels,
                                                         const uint32_t* __restrict__ unitFirst, const AlignRow* __restrict__ rows,
                                                         const long long* __restrict__ stepStart, const long long* __restrict__ chunkRow,
                                                         long long nRows, long long rowStride, const int* __restrict__ cols, int nCols,
                                                         long long hop, long long phase, long long padValue, int needSpan,
                                                         void* __restrict__ outp, long long total, int vecStore)
{
    constexpr int EL = I32 ? 4 : 2;
    const long long nLane = (total + EL - 1) / EL;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nLane; t += stride) {
        const long long e0 = t * EL;
        long long g, r, j;
        int q;
        dense_locate(e0, nCols, rowStride, stepStart, chunkRow, g, q, r, j);
        AlignRow row = rows[r];
        // the request of the step in hand, kept while the following elements stay inside it
        long long k = -1, kFirst = 0, kNext = 0, uFirst = 0, uNext = 0;
        FrameLabel lab = {0, 0u, 0, -1};
        long long v[EL];
#pragma unroll
        for (int i = 0; i < EL; ++i) {
            long long x = padValue;
            if (e0 + i < total) {
                if (rowStride == 0) while (j >= row.count && r + 1 < nRows) { ++r; j = 0; row = rows[r]; k = -1; }      // (rows without steps are stepped over)
                if (j < row.count) {
                    const long long s = phase + j * hop;
                    if (k < 0 || s < kFirst || s >= kNext) {
                        long long lo = 0, hi = row.nFrames;             // the last request dequeued on or before s
                        const TimelineReq* __restrict__ rq = req + row.frame0;
                        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (rq[mid].first <= s) lo = mid; else hi = mid; }
                        k = lo; kFirst = rq[k].first;
                        kNext = k + 1 < (long long)row.nFrames ? rq[k + 1].first : 0x7FFFFFFFFFFFFFFFll;
                        lab = labels[row.frame0 + k];
                        if (needSpan) {
                            const uint32_t* __restrict__ uf = unitFirst + row.unit0;
                            const uint32_t fa = uf[lab.unit], fb = uf[lab.unit + 1];      // (0 <= unit < nUnits: the set call refuses anything else)
                            uFirst = rq[fa].first;
                            uNext = fb < row.nFrames ? rq[fb].first : (long long)row.length;
                        }
                    }
                    switch (cols[q]) {
                    case kAlignPhoneme: x = lab.phoneme; break;
                    case kAlignStress: x = lab.flags & 3u; break;
                    case kAlignFlags: x = lab.flags; break;
                    case kAlignUnit: x = lab.unit; break;
                    case kAlignTextOffset: x = lab.textOffset; break;
                    case kAlignFrame: x = k; break;
                    case kAlignPosition: x = s - uFirst; break;
                    default: x = uNext - s; break;
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
        store16<typename std::conditional<I32, int, long long>::type>(outp, e0, total, vecStore, v);
    }
}

// Entry t of the table is (row, i): t / rowStride (padded; `padValue` in every column from the row's count on) or by bisection over
// entryStart[nRows + 1] (packed).  byFrame: entry i is frame i of the row's list; else unit i, frames unitFirst[i] .. unitFirst[i + 1] - 1.
__global__ void __launch_bounds__(256) klatt_align_units(const TimelineReq* __restrict__ req, const FrameLabel* __restrict__ labels,
                                                         const uint32_t* __restrict__ unitFirst, const AlignRow* __restrict__ rows,
                                                         const long long* __restrict__ entryStart, long long nRows, long long rowStride,
                                                         long long hop, long long phase, int byFrame, long long padValue,
                                                         long long* __restrict__ out, long long total)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        long long r, i;
        if (rowStride > 0) { r = t / rowStride; i = t - r * rowStride; }
        else packed_locate(t, entryStart, nRows, r, i);
        const AlignRow row = rows[r];
        long long* __restrict__ o = out + t * kUnitColumns;
        if (i >= row.count) {
            for (int c = 0; c < kUnitColumns; ++c) o[c] = padValue;
            continue;
        }
        const uint32_t* __restrict__ uf = unitFirst + row.unit0;
        const uint32_t fa = byFrame ? (uint32_t)i : uf[i], fb = byFrame ? (uint32_t)i + 1 : uf[i + 1];
        const TimelineReq* __restrict__ rq = req + row.frame0;
        const long long first = rq[fa].first, end = fb < row.nFrames ? rq[fb].first : (long long)row.length;
        uint32_t flags = 0, own = fa;
        bool found = false;
        for (uint32_t f = fa; f < fb; ++f) {
            const uint32_t fl = labels[row.frame0 + f].flags;
            flags |= fl;
            if (!found && !(fl & (kLabelGap | kLabelPuff))) { own = f; found = true; }
        }
        const FrameLabel lab = labels[row.frame0 + own];
        const long long before = align_steps_below(first, hop, phase);
        o[0] = lab.phoneme; o[1] = flags; o[2] = lab.textOffset;
        o[3] = first; o[4] = end - first;
        o[5] = before; o[6] = align_steps_below(end, hop, phase) - before;
    }
}

}  // namespace klatt
