// klatt_stage_window.h -- signal stages that keep a WINDOW of a row's most recent samples: the convolution and the spectrogram fed chunk by
// chunk (speechPlayer_batch_stageConvolve / stageSpectrogram, speechPlayer_stage_push; speechPlayer_spectrogramEmitted).
//
// The definition is in include/speechPlayer_batch.h ("Signal stages that keep a window").  Nothing per sample is restated here: the tap chain
// conv_step / conv_step4 / conv_finish and the block arithmetic of klatt_convolve.h, the transform's spec_* functions of klatt_spectrum.h,
// the reader's tile_x and the writer of klatt_tiles.h are called.  Nothing of the bookkeeping is either: klatt_stage.h has the counts of
// every kind (StageGeometry, stage_row_plan, the step grid StageFrames / stage_frames_emitted with its lemma), the virtual row (stage_where,
// stage_sample, stage_history_from_chunk) and the histories -- their layout, the row StageHistRow, klatt_stage_history_rows and
// klatt_stage_clear_rows, which resets the resampler's as well.  What this header adds is the two kinds' own: the convolution's block
// arithmetic at a stream index and the run reader, compiled for the host and for the device from one source (KLATT_RES_HD) and driven by
// the kernels and by the host model of tests/native/check_stage_window.cpp alike, and the two kernels with their argument structs.
//
//   The convolution Row r has K_r taps and keeps H_r = K_r - 1 samples.  A push emits y[N .. N' - 1] (+ K_r - 1 more where it ends the row
//                   with tail 1).  Output y[m] takes x[m - k], k = 0 .. K_r - 1: stream samples m - K_r + 1 .. m, none older than
//                   N - H_r.  The lemma of the export (klatt_convolve.h) applies: inserting or removing +-0 products changes nothing behind
//                   conv_finish's + 0.0f, so the sum over the virtual row [history | chunk | +0] is the statement's whether the history
//                   holds real samples or the +0 of a fresh row, and whole tap blocks whose inputs lie outside the stream's samples
//                   0 .. N' - 1 are skipped: conv_block_last / conv_block_skipped evaluated at the output's STREAM index N + t0 with the
//                   stream's length N' -- the virtual row's coordinates shifted by N - H_r --, so a fresh row's empty history still skips.
//   The spectrogram A row keeps the frame's before + after = nFft - 1 samples (klatt_stage.h, "The frames").
//   klatt_stage_convolve, klatt_stage_spectrogram
//                   Entry points on the bodies they share with klatt_convolve and klatt_spectrogram -- conv_rows<KEPT> of
//                   klatt_convolve.h, spec_rows of klatt_spectrum.h -- as klatt_stage_resample is on resample_rows<KEPT>
//                   (profiles/stage_window_kernels.txt: the whole-row exports measured no slower).  Each is the whole-row kernel's scheme whole.
//                   klatt_stage_convolve: 1024 outputs of a row per workgroup, tap blocks of 1024 in LDS, four outputs a lane,
//                   conv_step4, the writer; the reader is stage_read<-1>, tile_read<-1>'s counterpart on stage_sample.
//                   klatt_stage_spectrogram: one wavefront a step, four steps a workgroup, the XOR-swizzled LDS, the passes,
//                   spec_unpack / spec_value / spec_band / spec_scale, the 16-byte stores; the frame load is stage_sample, the step's
//                   centre phase + (M + j) hop in 64 bits.
#pragma once

#include "klatt_stage.h"
#include "klatt_convolve.h"
#include "klatt_spectrum.h"

namespace klatt {

constexpr long long kStageMaxHistory = 1ll << 27;      // float32 of history per buffer, all rows of a convolution or spectrogram stage together (512 MiB; there are two buffers)
constexpr long long kStageMaxStep = 1ll << 45;         // a hop or a phase above any row's 2^44 samples means the same as this one

// ---- the two kinds' own, for the host and the device -------------------------------------------------------------------------------------
// Samples of history a convolution row of K taps keeps
KLATT_RES_HD int stage_conv_history(long long K) { return (int)(K - 1); }
// The block at kb of a row's response, against the outputs t0 .. t0 + live - 1 of a push onto N consumed samples that makes them N2:
// conv_block_last / conv_block_skipped at the outputs' stream index
KLATT_RES_HD bool stage_conv_block_last(long long N, long long t0, int live, int kb) { return conv_block_last(N + t0, live, kb); }
KLATT_RES_HD bool stage_conv_block_skipped(long long N, long long N2, long long t0, int live, int kb, int taps) { return conv_block_skipped(N + t0, live, N2, kb, taps); }

// Lane `lane` of `lanes` of a run over the virtual row: element i stands for stream sample tile_source<DIR>(s0, i) (tile_read_lane's counterpart)
template <int DIR, typename In>
KLATT_RES_HD void stage_read_lane(float* xs, const float* hist, const In* chunk, long long N, int H, long long c, long long s0, int count, int lane, int lanes)
{
    for (int i = lane; i < count; i += lanes) xs[i] = stage_sample(hist, chunk, tile_source<DIR>(s0, i), N, H, c);
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace klatt {

// The workgroup's loads of a run over the virtual row
template <int DIR, typename In>
__device__ __forceinline__ void stage_read(float* xs, const float* __restrict__ hist, const In* __restrict__ chunk, long long N, int H, long long c, long long s0, int count, int tid)
{
    stage_read_lane<DIR>(xs, hist, chunk, N, H, c, s0, count, tid, 256);
}

struct StageConvArgs {
    const void* in;                      // the chunk's data: int16_t or float, as the kernel's In says
    const StageHistRow* rows;
    TileOut tile;
    const float* taps;                   // the responses back to back
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_stage_convolve(const StageConvArgs A)
{
    conv_rows<true, F32, In>(A, [&](float* xr, const In* __restrict__ chunk, const StageHistRow& row, long long s0, int count, int tid) {
        stage_read<-1>(xr, A.hist + row.hist, chunk, row.N, (int)row.H, row.len, s0, count, tid);
    });
}

struct StageSpecArgs {
    SpecArgs s;                          // klatt_spectrogram's, `rows` unused: the table, the step grid, the plan's arrays, the output
    const StageHistRow* rows;
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(64 * kSpecWaves) klatt_stage_spectrogram(const StageSpecArgs S)
{
    const SpecArgs& A = S.s;
    const int M = 1 << (A.logN - 1);
    spec_rows<F32>(A, S.rows, [](const StageHistRow& row) { return row.outLen; },
                   [&](const StageHistRow& row, long long j) { return A.phase + (row.M + j) * A.hop - M; },      // step M + j of the row's stream
                   [&](const StageHistRow& row, long long t) { return stage_sample(S.hist + row.hist, static_cast<const In*>(A.in) + row.src, t, row.N, (int)row.H, row.len); });
}

}  // namespace klatt
#endif
