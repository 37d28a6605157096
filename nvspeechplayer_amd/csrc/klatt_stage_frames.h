// klatt_stage_frames.h -- signal stages on the step grid: the linear-prediction analysis and the pitch (YIN) fed chunk by chunk
// (speechPlayer_batch_stageLpc / stagePitch, speechPlayer_stage_push; speechPlayer_lpcEmitted / pitchEmitted).
//
// The definition is in include/speechPlayer_batch.h ("Signal stages on the step grid").  Nothing per sample is restated here: the window
// product, lpc_term, the lane partials and their tree, lpc_lagged, lpc_levinson and lpc_put_fields of klatt_lpc.h, pitch_lane_diff, the
// scan, pitch_cmnd, pitch_lane_choice, pitch_better and pitch_put_fields of klatt_pitch.h and the writer of klatt_tiles.h are called, through
// the bodies the whole-row kernels are entry points of -- lpc_rows and pitch_rows.  Nothing of the bookkeeping is either: klatt_stage.h has
// the step grid (StageFrames, stage_lpc_frames, stage_pitch_frames, stage_frames_emitted with its lemma), the row plan, the virtual row
// (stage_sample) and the histories with StageHistRow, klatt_stage_history_rows and klatt_stage_clear_rows.  tests/native/
// check_stage_frames.cpp drives that bookkeeping and the host's frame statements chunk by chunk against lpc_host and pitch_host.
//
//   klatt_stage_lpc, klatt_stage_pitch
//                   Entry points on lpc_rows<F32> and pitch_rows<F32>, as klatt_stage_spectrogram is on spec_rows
//                   (profiles/stage_frames.txt: the whole-row exports measured no slower, their registers unchanged).  What differs from
//                   klatt_lpc and klatt_pitch is what differs for the spectrogram stage: a row's steps are the push's (row.outLen); step
//                   j of the push is step M + j of the row's stream, its frame's first sample phase + (M + j) hop - floor(n / 2) in 64
//                   bits, n the frame's length (nWin; W + lagMax); the reader is stage_sample on [history | chunk | +0].  The output's
//                   steps are located by dense_locate over the push's own step table, so a group of 64 (16) steps may end one row and
//                   begin the next, rows with unlike M among them.
#pragma once

#include "klatt_stage.h"
#include "klatt_lpc.h"
#include "klatt_pitch.h"

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace klatt {

struct StageLpcArgs {
    LpcArgs s;                           // klatt_lpc's, `rows` unused: the table, the step grid, the plan and its arrays, the output
    const StageHistRow* rows;
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_stage_lpc(const StageLpcArgs S)
{
    const LpcArgs& A = S.s;
    lpc_rows<F32>(A, S.rows, [](const StageHistRow& row) { return row.outLen; },
                  [&](const StageHistRow& row, long long j) { return A.phase + (row.M + j) * A.hop - A.nWin / 2; },      // step M + j of the row's stream
                  [&](const StageHistRow& row, long long t) { return stage_sample(S.hist + row.hist, static_cast<const In*>(A.in) + row.src, t, row.N, (int)row.H, row.len); });
}

struct StagePitchArgs {
    PitchArgs s;                         // klatt_pitch's, `rows` unused
    const StageHistRow* rows;
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_stage_pitch(const StagePitchArgs S)
{
    const PitchArgs& A = S.s;
    pitch_rows<F32>(A, S.rows, [](const StageHistRow& row) { return row.outLen; },
                    [&](const StageHistRow& row, long long j) { return A.phase + (row.M + j) * A.hop - (A.nWin + A.lagMax) / 2; },
                    [&](const StageHistRow& row, long long t) { return stage_sample(S.hist + row.hist, static_cast<const In*>(A.in) + row.src, t, row.N, (int)row.H, row.len); });
}

}  // namespace klatt
#endif
