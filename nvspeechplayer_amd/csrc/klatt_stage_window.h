// klatt_stage_window.h -- signal stages that keep a WINDOW of a row's most recent samples: the convolution and the spectrogram fed chunk by
// chunk (speechPlayer_batch_stageConvolve / stageSpectrogram, speechPlayer_stage_push; speechPlayer_spectrogramEmitted).
//
// The definition is in include/speechPlayer_batch.h ("Signal stages that keep a window").  Nothing per sample is restated here: the tap chain
// conv_step / conv_step4 / conv_finish and the block arithmetic of klatt_convolve.h, the transform's spec_* functions of klatt_spectrum.h,
// the reader's tile_x and the writer of klatt_tiles.h, and the virtual row of klatt_stage.h (stage_where, stage_sample,
// stage_history_from_chunk) are called.  What this header adds is the resampler stage's mechanism with a history length PER ROW -- compiled
// for the host and for the device from one source (KLATT_RES_HD) and driven by the kernels, by the entry points and by the host model of
// tests/native/check_stage_window.cpp alike -- and the two kernels on it.
//
//   The frames      A frame (before, after) of step j is the samples c_j - before .. c_j + after around its centre c_j = phase + j hop
//                   (stage_frame_centre).  The spectrogram's frame is (nFft / 2, nFft / 2 - 1); LPC's (floor(nWin / 2), nWin - 1 -
//                   floor(nWin / 2)) and YIN's fit the same bookkeeping.  Open, the steps emitted after N samples are those whose whole
//                   frame lies at or before sample N - 1:  c_j + after <= N - 1  <=>  j <= (N - after - 1 - phase) / hop, so
//                   E_open(N) = 0 where N - after - 1 - phase < 0 and floor((N - after - 1 - phase) / hop) + 1 otherwise.  Ended, the
//                   statement's count ceil((N - phase) / hop) (0 where N <= phase), the samples past N - 1 being +0 as the statement has
//                   them.  A push emits E(N', ended) - M (stage_frames_emitted).  N <= 2^44, hop and phase <= 2^45: 64 bits hold it all.
//   The lemma       before + after samples of history suffice, whatever hop and phase are.  Step M, the first not emitted with N
//                   consumed, has c_M + after > N - 1, so its oldest sample c_M - before >= N - (before + after); c_j does not decrease
//                   with j, so no later step reaches further back.  A hop above the frame's length skips samples; the history then holds
//                   some that no step reads, which costs nothing.
//   The convolution Row r has K_r taps and keeps H_r = K_r - 1 samples.  A push emits y[N .. N' - 1] (+ K_r - 1 more where it ends the row
//                   with tail 1).  Output y[m] takes x[m - k], k = 0 .. K_r - 1: stream samples m - K_r + 1 .. m, none older than
//                   N - H_r.  The export's lemma (klatt_convolve.h) applies: inserting or removing +-0 products changes nothing behind
//                   conv_finish's + 0.0f, so the sum over the virtual row [history | chunk | +0] is the statement's whether the history
//                   holds real samples or the +0 of a fresh row, and whole tap blocks whose inputs lie outside the stream's samples
//                   0 .. N' - 1 are skipped: conv_block_last / conv_block_skipped evaluated at the output's STREAM index N + t0 with the
//                   stream's length N' -- the virtual row's coordinates shifted by N - H_r --, so a fresh row's empty history still skips.
//   The window      As klatt_stage.h's: the next history is the last H_r of [history | chunk], zeros for an ended row, written to the
//                   OTHER of two buffers by klatt_stage_history_rows -- klatt_stage_history with a row's length and its first element
//                   read from the row table, since rows differ.  The host swaps the buffers after every launch of the push is queued.
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

constexpr int kStageConvolve = 3, kStageSpectrogram = 4;
constexpr long long kStageMaxHistory = 1ll << 27;      // float32 of history per buffer, all rows together (512 MiB; there are two buffers)
constexpr long long kStageMaxStep = 1ll << 45;         // a hop or a phase above any row's 2^44 samples means the same as this one

// ---- the bookkeeping, for the host and the device ---------------------------------------------------------------------------------------
// A step grid with a frame around every centre
struct StageFrames { long long before = 0, after = 0, hop = 1, phase = 0; };
KLATT_RES_HD StageFrames stage_spec_frames(int nFft, long long hop, long long phase) { StageFrames f; f.before = nFft / 2; f.after = nFft / 2 - 1; f.hop = hop; f.phase = phase; return f; }
KLATT_RES_HD int stage_frame_history(const StageFrames& f) { return (int)(f.before + f.after); }
KLATT_RES_HD long long stage_frame_centre(const StageFrames& f, long long j) { return f.phase + j * f.hop; }
// Steps emitted once N samples are consumed, open (the whole frame at or before sample N - 1) or ended (the statement's count)
KLATT_RES_HD long long stage_frames_emitted(const StageFrames& f, long long N, bool ended)
{
    if (ended) return N > f.phase ? (N - f.phase + f.hop - 1) / f.hop : 0;
    const long long a = N - f.after - 1 - f.phase;
    return a < 0 ? 0 : a / f.hop + 1;
}
// Samples of history a convolution row of K taps keeps
KLATT_RES_HD int stage_conv_history(long long K) { return (int)(K - 1); }
// The block at kb of a row's response, against the outputs t0 .. t0 + live - 1 of a push onto N consumed samples that makes them N2:
// conv_block_last / conv_block_skipped at the outputs' stream index
KLATT_RES_HD bool stage_conv_block_last(long long N, long long t0, int live, int kb) { return conv_block_last(N + t0, live, kb); }
KLATT_RES_HD bool stage_conv_block_skipped(long long N, long long N2, long long t0, int live, int kb, int taps) { return conv_block_skipped(N + t0, live, N2, kb, taps); }

// What a window stage is, as far as the counts go: a convolution row's taps come with the row
struct StageWindowGeometry { int kind = kStageConvolve, tail = 0; StageFrames frames; };
// The outputs of a push of c samples, ended or not, onto a row at (N, M) of K taps (a convolution's); false: c is negative or the row
// would pass 2^44 samples
KLATT_RES_HD bool stage_window_row_plan(const StageWindowGeometry& g, long long K, long long N, long long M, long long c, bool ended, long long& out)
{
    out = 0;
    if (c < 0 || c > kResampleMaxLength - N) return false;
    if (g.kind == kStageConvolve) out = c + (ended && g.tail ? K - 1 : 0);
    else out = stage_frames_emitted(g.frames, N + c, ended) - M;
    return true;
}

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

// A row of a window stage's push: first element and samples of its chunk; the samples it has consumed and the outputs it has emitted
// before; the outputs of this push; their first element in the output (a convolution's); whether the push ends it; its history's first
// element in either buffer and its length; its response's first tap (a convolution's, of H + 1 taps)
struct StageWinRow { long long src, len, N, M, outLen, dst, ended, hist, H, irAt; };

// The workgroup's loads of a run over the virtual row
template <int DIR, typename In>
__device__ __forceinline__ void stage_read(float* xs, const float* __restrict__ hist, const In* __restrict__ chunk, long long N, int H, long long c, long long s0, int count, int tid)
{
    stage_read_lane<DIR>(xs, hist, chunk, N, H, c, s0, count, tid, 256);
}

// The next history of every row, into the buffer this push does not read: the last H of [history | chunk], zeros for an ended row.
// Workgroups (x, y): the rows y, y + gridDim.y, ..; of a row the elements x 256 + lane, + gridDim.x 256, ..
template <typename In>
__global__ void __launch_bounds__(256) klatt_stage_history_rows(const void* in, const StageWinRow* __restrict__ rows, long long nRows, const float* __restrict__ from,
                                                                float* __restrict__ to)
{
    for (long long r = blockIdx.y; r < nRows; r += gridDim.y) {
        const StageWinRow row = rows[r];
        const int H = (int)row.H;
        for (int j = blockIdx.x * 256 + threadIdx.x; j < H; j += gridDim.x * 256) {
            float v = 0.0f;
            if (!row.ended) {
                long long at;
                if (stage_history_from_chunk(j, H, row.len, at)) v = tile_x(static_cast<const In*>(in)[row.src + at]);
                else v = from[row.hist + at];
            }
            to[row.hist + j] = v;
        }
    }
}

// +0 into the history of the chosen rows (rows null: all): row r's is at[r] .. at[r + 1] - 1
__global__ void __launch_bounds__(256) klatt_stage_clear_rows(const unsigned char* __restrict__ rows, const long long* __restrict__ at, long long nRows, float* __restrict__ state)
{
    for (long long r = blockIdx.y; r < nRows; r += gridDim.y) {
        if (rows && !rows[r]) continue;
        const long long a = at[r], b = at[r + 1];
        for (long long e = a + blockIdx.x * 256 + threadIdx.x; e < b; e += gridDim.x * 256) state[e] = 0.0f;
    }
}

struct StageConvArgs {
    const void* in;                      // the chunk's data: int16_t or float, as the kernel's In says
    const StageWinRow* rows;
    TileOut tile;
    const float* taps;                   // the responses back to back
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_stage_convolve(const StageConvArgs A)
{
    conv_rows<true, F32, In>(A, [&](float* xr, const In* __restrict__ chunk, const StageWinRow& row, long long s0, int count, int tid) {
        stage_read<-1>(xr, A.hist + row.hist, chunk, row.N, (int)row.H, row.len, s0, count, tid);
    });
}

struct StageSpecArgs {
    SpecArgs s;                          // klatt_spectrogram's, `rows` unused: the table, the step grid, the plan's arrays, the output
    const StageWinRow* rows;
    const float* hist;                   // the buffer this push reads
};

template <bool F32, typename In>
__global__ void __launch_bounds__(64 * kSpecWaves) klatt_stage_spectrogram(const StageSpecArgs S)
{
    const SpecArgs& A = S.s;
    const int M = 1 << (A.logN - 1);
    spec_rows<F32>(A, S.rows, [](const StageWinRow& row) { return row.outLen; },
                   [&](const StageWinRow& row, long long j) { return A.phase + (row.M + j) * A.hop - M; },      // step M + j of the row's stream
                   [&](const StageWinRow& row, long long t) { return stage_sample(S.hist + row.hist, static_cast<const In*>(A.in) + row.src, t, row.N, (int)row.H, row.len); });
}

}  // namespace klatt
#endif
