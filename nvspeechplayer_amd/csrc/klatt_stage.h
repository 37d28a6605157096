// klatt_stage.h -- signal stages: the resampler, the biquad filter and the codecs fed chunk by chunk, with the state that survives a call
// (speechPlayer_batch_stageResample / stageFilter / stageCode, speechPlayer_stage_push; speechPlayer_resampleEmitted), and what all kinds share.
//
// The definition is in include/speechPlayer_batch.h ("Signal stages").  Nothing per sample is restated here: the resampler's res_locate /
// res_taps / res_value, the filter's filter_section / filter_finish, the codecs' adpcm_encode and G.711 laws and the reader's tile_x are the
// functions of klatt_resample.h, klatt_filter.h, klatt_codec.h and klatt_tiles.h, called.  What this header adds is the bookkeeping of ALL
// seven kinds, compiled for the host and for the device from one source (KLATT_RES_HD) and driven by the kernels, by the entry points and by
// the host models of tests/native/check_stage.cpp and check_stage_window.cpp alike, and the kernels of the resampler, the filter and ADPCM.
//
//   Who owns what   here: the kind constants, StageGeometry and stage_row_plan (what a push emits, every kind); the step grid (StageFrames);
//                   the virtual row (stage_where, stage_sample, stage_history_from_chunk); the histories' layout with StageHistRow,
//                   klatt_stage_history_rows and klatt_stage_clear_rows; the resampler's StageResRow, klatt_stage_resample and
//                   klatt_stage_history; the filter's and ADPCM's lane state, klatt_stage_filter, klatt_stage_adpcm, klatt_stage_clear.
//                   klatt_stage_window.h: the convolution's block arithmetic, stage_read_lane / stage_read, the two kinds' kernels.
//                   klatt_stage_frames.h: the LPC and the pitch stage's kernels, entry points on lpc_rows and pitch_rows.
//   The counts      A row has consumed N samples and emitted M outputs since its start (its creation, its last end or its last reset).  A
//                   push of c samples makes N' = N + c.  The resampler, open, emits the outputs m whose taps n0(m) - Z + 1 .. n0(m) + Z,
//                   n0(m) = floor(m down / up), all lie at or before sample N' - 1:  n0(m) + Z <= N' - 1  <=>  m down < (N' - Z) up  <=>
//                   m < (N' - Z) up / down, so M' = ceil(max(N' - Z, 0) up / down) = stage_res_emitted.  Ended, it emits the statement's
//                   count ceil(N' up / down), the samples past N' - 1 being +0 as the statement has them.  N <= 2^44 and up <= 2^12, so the
//                   product stays in 64 bits on both sides.  Equal rates filter nothing: Z = 0 there, M = N.
//   The lemma       2 Z - 1 samples of history suffice.  Output M, the first not yet emitted with N consumed, has n0(M) + Z > N - 1, so
//                   its oldest tap n0(M) - Z + 1 >= N - 2 Z + 1; n0 does not decrease with m, so no later output reaches further back.  The
//                   samples N - 2 Z + 1 .. N - 1 are 2 Z - 1 = stage_history(Z) values, float32 as tile_x gave them, +0 before sample 0.
//   The frames      A frame (before, after) of step j is the samples c_j - before .. c_j + after around its centre c_j = phase + j hop
//                   (stage_frame_centre).  The spectrogram's frame is (nFft / 2, nFft / 2 - 1) (stage_spec_frames); LPC's is
//                   (floor(nWin / 2), nWin - 1 - floor(nWin / 2)) (stage_lpc_frames) and YIN's the same of its nWin + lagMax samples
//                   (stage_pitch_frames), as lpc_host and pitch_host place a frame's first sample at c_j - floor(n / 2).  Open, the steps emitted after N samples are those whose whole
//                   frame lies at or before sample N - 1:  c_j + after <= N - 1  <=>  j <= (N - after - 1 - phase) / hop, so
//                   E_open(N) = 0 where N - after - 1 - phase < 0 and floor((N - after - 1 - phase) / hop) + 1 otherwise.  Ended, the
//                   statement's count ceil((N - phase) / hop) (0 where N <= phase), the samples past N - 1 being +0 as the statement has
//                   them.  A push emits E(N', ended) - M (stage_frames_emitted).  N <= 2^44, hop and phase <= 2^45: 64 bits hold it all.
//                   before + after samples of history suffice, whatever hop and phase are: step M, the first not emitted with N
//                   consumed, has c_M + after > N - 1, so its oldest sample c_M - before >= N - (before + after); c_j does not decrease
//                   with j, so no later step reaches further back.  (A hop above the frame's length skips samples that the history holds.)
//   The virtual row [history | chunk | +0]: sample n of the row's stream is element v = n - (N - H) of it, H the samples of history the
//                   row keeps -- 2 Z - 1, a convolution row's K_r - 1, a frame's before + after; 0 at equal rates -- (stage_where): below 0
//                   it is +0 (a sample before the start that the history no longer holds: by the lemma no output of the push needs it),
//                   below H the history's, below H + c the chunk's, beyond it +0 -- needed by an ended row's last outputs alone.
//   The window      The next history is the last H elements of [history | chunk]: element j is element c + j of it
//                   (stage_history_from_chunk), all zeros for an ended row.  It is written to the OTHER of two buffers by a kernel of its own
//                   (klatt_stage_history_rows; the resampler's klatt_stage_history), so no workgroup writes what another reads; the host
//                   swaps the buffers once the push is queued.  Row r's history lies at histAt[r] of either buffer.  StageHistRow carries
//                   that place and the length, since a convolution's rows differ; the resampler's are uniform, r H, and its pushes leave
//                   them out of the row (StageResRow).  klatt_stage_clear_rows puts +0 into the chosen rows' histories (a reset), all kinds'.
//   klatt_stage_resample
//                   resample_rows<KEPT = true> of klatt_resample.h, the one body it shares with klatt_resample: that kernel's tiling --
//                   kResampleTile outputs a workgroup, spans whose inputs fit kResampleIn floats of LDS, the transposed table, the writer
//                   of klatt_tiles.h.  The entry point here hands it the reader of the virtual row (stage_sample) in place of tile_read,
//                   and KEPT makes a span's first output the row's global index M + t0, located in 64 bits (the phase column as well);
//                   addresses are relative to the chunk and to the row's place in the output.
//   klatt_stage_filter, klatt_stage_adpcm
//                   Siblings of klatt_filter and klatt_code_adpcm, not entry points on one body: merged, three rows of the timing probes
//                   lay above the parent's maximum (profiles/stage_kernels_one_body.txt), so the loops stay written twice.
//                   klatt_filter's and klatt_code_adpcm's scheme whole -- a lane per row, tiles transposed through LDS, coefficients and
//                   states in registers, the buckets with identity padding -- with the states loaded from the stage before the first sample
//                   and stored behind the last.  Those kernels keep stepping on zeros past a row's own samples while the group's longest
//                   row goes on, which is harmless for a whole row and wrong for a state that is kept: here a tile that some lane's row
//                   ends in (a wave-uniform test) runs steps that commit the state only while t < the row's own count, so what is stored is
//                   the state after exactly c samples (c + tail for an ended filter row, which is then stored as +0; val = idx = 0).
//                   Identity padding sits behind the real sections, so the real sections' states are exact; the padding's are never stored.
//                   (Their state is uniform, 16 and 2 dwords a row, and updated in place: the flat klatt_stage_clear resets it.)
//   Out of scope    The tempo export and the LPC residual chunk by chunk (a sample's frame is the nearest centre: it needs frames still to
//                   come); a mix stage; saving a stage's state to the host; NodePlayer; a fused kernel for a chain of stages.  (A kind on
//                   the step grid is a plan, stage_has_frames and a kernel entry point on the history above: klatt_stage_frames.h.)
#pragma once

#include "klatt_codec.h"

namespace klatt {

constexpr long long kStageMaxRows = 1ll << 20;
constexpr int kStageResample = 0, kStageFilter = 1, kStageCode = 2, kStageConvolve = 3, kStageSpectrogram = 4, kStageLpc = 5, kStagePitch = 6;
constexpr int kStageFilterState = 2 * kFilterMaxSections;      // floats of a filter stage's row: s1, s2 of section j at 2 j, 2 j + 1

// ---- the bookkeeping, for the host and the device ---------------------------------------------------------------------------------------
// Samples of history a resampler row keeps
KLATT_RES_HD int stage_history(int Z) { return Z > 0 ? 2 * Z - 1 : 0; }
// ceil(n up / down) for 0 <= n <= 2^44, up <= 2^12: the product stays in 64 bits
KLATT_RES_HD long long stage_ceil(long long n, int up, int down) { return (n * (long long)up + (long long)(down - 1)) / (long long)down; }
// Outputs a resampler row has emitted once it has consumed N samples, open or ended (Z 0: equal rates)
KLATT_RES_HD long long stage_res_emitted(long long N, int Z, int up, int down, bool ended)
{
    return stage_ceil(ended ? N : (N > Z ? N - Z : 0), up, down);
}
// Where sample n of a row's stream lies for a push of c samples onto N consumed ones with H of history: 0 nowhere (+0), 1 element `at` of
// the history, 2 element `at` of the chunk
KLATT_RES_HD int stage_where(long long n, long long N, int H, long long c, long long& at)
{
    const long long v = n - (N - H);
    at = 0;
    if (v < 0) return 0;
    if (v < H) { at = v; return 1; }
    if (v - H < c) { at = v - H; return 2; }
    return 0;
}
// ... and its value: the reader of the virtual row.  Nothing outside the history and the chunk is loaded.
template <typename In> KLATT_RES_HD float stage_sample(const float* hist, const In* chunk, long long n, long long N, int H, long long c)
{
    long long at;
    const int part = stage_where(n, N, H, c, at);
    return part == 1 ? hist[at] : part == 2 ? tile_x(chunk[at]) : 0.0f;
}
// Element j of the next history, the last H of [history | chunk]: true with the chunk's element `at`, false with the history's
KLATT_RES_HD bool stage_history_from_chunk(int j, int H, long long c, long long& at)
{
    const long long v = c + j;
    if (v < H) { at = v; return false; }
    at = v - H;
    return true;
}

// A step grid with a frame around every centre
struct StageFrames { long long before = 0, after = 0, hop = 1, phase = 0; };
KLATT_RES_HD StageFrames stage_spec_frames(int nFft, long long hop, long long phase) { StageFrames f; f.before = nFft / 2; f.after = nFft / 2 - 1; f.hop = hop; f.phase = phase; return f; }
// LPC's frame of nWin samples and YIN's of nWin + lagMax around the centre, as lpc_host and pitch_host place them: t0 = c - n / 2
KLATT_RES_HD StageFrames stage_frames_of(int n, long long hop, long long phase) { StageFrames f; f.before = n / 2; f.after = n - 1 - n / 2; f.hop = hop; f.phase = phase; return f; }
KLATT_RES_HD StageFrames stage_lpc_frames(int nWin, long long hop, long long phase) { return stage_frames_of(nWin, hop, phase); }
KLATT_RES_HD StageFrames stage_pitch_frames(int nWin, int lagMax, long long hop, long long phase) { return stage_frames_of(nWin + lagMax, hop, phase); }
KLATT_RES_HD int stage_frame_history(const StageFrames& f) { return (int)(f.before + f.after); }
KLATT_RES_HD long long stage_frame_centre(const StageFrames& f, long long j) { return f.phase + j * f.hop; }
// Steps emitted once N samples are consumed, open (the whole frame at or before sample N - 1) or ended (the statement's count)
KLATT_RES_HD long long stage_frames_emitted(const StageFrames& f, long long N, bool ended)
{
    if (ended) return N > f.phase ? (N - f.phase + f.hop - 1) / f.hop : 0;
    const long long a = N - f.after - 1 - f.phase;
    return a < 0 ? 0 : a / f.hop + 1;
}

// What a stage is, as far as the counts go.  Z 0: a resampler at equal rates.  tail: the filter's samples, the convolution's 0 or 1.
// frames: the spectrogram's, LPC's, the pitch's.  A convolution row's taps come with the row, as its history + 1.
struct StageGeometry { int kind = 0, up = 1, down = 1, Z = 0; long long tail = 0; StageFrames frames; };
// The kinds on the step grid: their outputs are steps, [step][columns], and a row keeps its frame's before + after samples
KLATT_RES_HD bool stage_has_frames(int kind) { return kind == kStageSpectrogram || kind == kStageLpc || kind == kStagePitch; }
// The kinds whose rows keep a history of their most recent samples (a resampler's at equal rates has length 0); the others keep lane state
KLATT_RES_HD bool stage_keeps_history(int kind) { return kind == kStageResample || kind == kStageConvolve || stage_has_frames(kind); }
// The outputs of a push of c samples, ended or not, onto a row at (N, M) that keeps H samples of history (read for the convolution, whose
// H is K - 1, alone); false: c is negative or the row would pass 2^44 samples
KLATT_RES_HD bool stage_row_plan(const StageGeometry& g, long long H, long long N, long long M, long long c, bool ended, long long& out)
{
    out = 0;
    if (c < 0 || c > kResampleMaxLength - N) return false;
    if (g.kind == kStageResample) out = stage_res_emitted(N + c, g.Z, g.up, g.down, ended) - M;
    else if (g.kind == kStageFilter) out = c + (ended ? g.tail : 0);
    else if (g.kind == kStageConvolve) out = c + (ended && g.tail ? H : 0);
    else if (stage_has_frames(g.kind)) out = stage_frames_emitted(g.frames, N + c, ended) - M;
    else out = c;
    return true;
}
// ... and the row's counts behind it: a fresh row after an end
KLATT_RES_HD void stage_row_advance(long long& N, long long& M, long long c, bool ended, long long out)
{
    if (ended) { N = 0; M = 0; }
    else { N += c; M += out; }
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace klatt {

// A row of a push onto a stage that keeps a history: first element and samples of its chunk; the samples it has consumed and the outputs
// it has emitted before; the outputs of this push; their first element in the output (the spectrogram's are located by its own table);
// whether the push ends it; its history's first element in either buffer and its length; its response's first tap (a convolution's, of
// H + 1 taps; 0 otherwise)
struct StageHistRow { long long src, len, N, M, outLen, dst, ended, hist, H, irAt; };

// The next history of every row, into the buffer this push does not read: the last H of [history | chunk], zeros for an ended row.
// Workgroups (x, y): the rows y, y + gridDim.y, ..; of a row the elements x 256 + lane, + gridDim.x 256, ..
template <typename In>
__global__ void __launch_bounds__(256) klatt_stage_history_rows(const void* in, const StageHistRow* __restrict__ rows, long long nRows, const float* __restrict__ from,
                                                                float* __restrict__ to)
{
    for (long long r = blockIdx.y; r < nRows; r += gridDim.y) {
        const StageHistRow row = rows[r];
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

// A resampler row of a push: StageHistRow's first seven fields; row r's history is the 2 Z - 1 samples at r (2 Z - 1).  A row table is
// staged and uploaded at every push: with 80 bytes a row for these 56, 16384 rows x 256 samples took 17 % longer (profiles/stage_one_history.txt)
struct StageResRow { long long src, len, N, M, outLen, dst, ended; };

struct StageResArgs {
    const void* in;                      // the chunk's data: int16_t or float, as the kernel's In says
    const StageResRow* rows;
    TileOut tile;
    const float* hT;                     // [taps][up]
    const float* hist;                   // [row][2 Z - 1]: the buffer this push reads
    int up, down, Z, span;
};

template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_stage_resample(const StageResArgs A)
{
    const int H = stage_history(A.Z);
    resample_rows<true, F32, In>(A, [&](float* xin, const In* __restrict__ chunk, long long r, const StageResRow& row, long long first, int count, int tid) {
        const float* __restrict__ hist = A.hist + r * H;
        for (int i = tid; i < count; i += 256) xin[i] = stage_sample(hist, chunk, first + i, row.N, H, row.len);
    });
}

// klatt_stage_history_rows for the resampler's uniform histories and 56-byte rows: one lane per history element, flat over all rows
template <typename In>
__global__ void __launch_bounds__(256) klatt_stage_history(const void* in, const StageResRow* __restrict__ rows, long long nRows, int H,
                                                           const float* __restrict__ from, float* __restrict__ to)
{
    const long long total = nRows * H, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long r = e / H;
        const int j = (int)(e - r * H);
        const StageResRow row = rows[r];
        float v = 0.0f;
        if (!row.ended) {
            long long at;
            if (stage_history_from_chunk(j, H, row.len, at)) v = tile_x(static_cast<const In*>(in)[row.src + at]);
            else v = from[r * H + at];
        }
        to[e] = v;
    }
}

// +0 into the lane state of the chosen rows (rows null: all) of a filter or ADPCM stage: perRow dwords each, uniform and updated in place, so a flat clear suits it
__global__ void __launch_bounds__(256) klatt_stage_clear(const unsigned char* __restrict__ rows, long long nRows, int perRow, uint32_t* __restrict__ state)
{
    const long long total = nRows * perRow, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride)
        if (!rows || rows[e / perRow]) state[e] = 0u;
}

// A row of a filter or ADPCM stage's push: klatt_filter's row, the stage's row whose state it carries, and whether the push ends it
struct StageLaneRow : FilterRow { long long state, ended; };

struct StageFilterArgs {
    const void* in;                      // the chunk's data: int16_t or float, as the kernel's In says
    const StageLaneRow* rows;            // the packed table
    const FilterGroup* groups;           // the groups of this launch's bucket
    long long nGroups;
    const FilterSection* sections;       // the filters back to back
    long long rowStride;                 // the padded form: a row's width
    void* out;
    float* state;                        // [row][kStageFilterState]
};

template <int K, bool F32, typename In>
__global__ void __launch_bounds__(kFilterLanes) klatt_stage_filter(const StageFilterArgs A)
{
    using T = TileValue<F32>;
    constexpr int TILE = kFilterTile;
    __shared__ __attribute__((aligned(16))) float region[kFilterLanes * kFilterPitch];
    __shared__ __attribute__((aligned(16))) long long where[kFilterLanes][2];
    const int lane = threadIdx.x;
    float* const mine = region + lane * kFilterPitch;
    T* const staged = reinterpret_cast<T*>(mine);
    const In* __restrict__ in = static_cast<const In*>(A.in);
    for (long long g = blockIdx.x; g < A.nGroups; g += gridDim.x) {
        const FilterGroup G = A.groups[g];
        const StageLaneRow me = A.rows[G.first + lane];
        float* const kept = A.state + me.state * kStageFilterState;      // (a filler has no sections and touches nothing)
        FilterSection c[K];
        float s1[K], s2[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool real = j < me.sections;
            c[j] = real ? A.sections[me.secAt + j] : kFilterIdentity;
            s1[j] = real ? kept[2 * j] : 0.0f;
            s2[j] = real ? kept[2 * j + 1] : 0.0f;
        }
        where[lane][0] = me.sections ? me.dst : -1;
        where[lane][1] = me.outLen;
        const long long width = A.rowStride > 0 ? A.rowStride : G.outMost;
        In next[kFilterLanes];
        filter_load_rows(next, in, me.src, me.len, 0, lane);
        bool zeroed = false;
        for (long long t0 = 0; t0 < width; t0 += TILE) {
            if (t0 < G.outMost) {
                __syncthreads();                                   // the tile before has left the region
#pragma unroll
                for (int q = 0; q < kFilterLanes; ++q) region[q * kFilterPitch + lane] = tile_x(next[q]);
                // the next tile's loads, in flight during the section steps (none where no row of the group reaches it)
                if (t0 + TILE < G.inMost) filter_load_rows(next, in, me.src, me.len, t0 + TILE, lane);
                else {
#pragma unroll
                    for (int q = 0; q < kFilterLanes; ++q) next[q] = (In)0;
                }
                __syncthreads();
                const long long live = me.outLen - t0;             // steps of the tile that are the lane's row's own; the rest is padding
                if (__all(live >= TILE || me.sections == 0)) {     // (wave-uniform) no row of the group ends in this tile: klatt_filter's steps (a filler stores nothing)
                    for (int t = 0; t < TILE; ++t) {
                        float x = mine[t];
#pragma unroll
                        for (int j = 0; j < K; ++j) x = filter_section(c[j], x, s1[j], s2[j]);
                        staged[t] = res_value<F32>(filter_finish(x));
                    }
                } else {                                           // a step past the row's own count leaves its state as it is
                    for (int t = 0; t < TILE; ++t) {
                        const bool on = t < live;
                        float x = mine[t];
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            float a = s1[j], b = s2[j];
                            x = filter_section(c[j], x, a, b);
                            s1[j] = on ? a : s1[j];
                            s2[j] = on ? b : s2[j];
                        }
                        staged[t] = on ? res_value<F32>(filter_finish(x)) : (T)0;
                    }
                }
                __syncthreads();
            } else if (!zeroed) {                                  // (padded rows past the group's longest: +0 without arithmetic)
                __syncthreads();
                for (int t = 0; t < TILE; ++t) mine[t] = 0.0f;
                zeroed = true;
                __syncthreads();
            }
            filter_store_rows<T>(A.out, where, A.rowStride, t0, region, lane);
        }
        // the state behind exactly the row's own steps; +0 behind an end
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < me.sections) {
                kept[2 * j] = me.ended ? 0.0f : s1[j];
                kept[2 * j + 1] = me.ended ? 0.0f : s2[j];
            }
        __syncthreads();                                           // the last tile has left before the next group's first
    }
}

struct StageAdpcmArgs {
    const void* in;                      // as StageFilterArgs'
    const StageLaneRow* rows;            // the packed table (a section each, fillers none)
    const FilterGroup* groups;
    long long nGroups;
    long long rowStride;
    void* decoded;                       // or null, as OUT says
    uint8_t* codes;
    int* state;                          // [row][2]: val, idx
};

template <int OUT, bool F32, typename In>
__global__ void __launch_bounds__(kFilterLanes) klatt_stage_adpcm(const StageAdpcmArgs A)
{
    using T = TileValue<F32>;
    constexpr int TILE = kFilterTile, PITCH = codec_pitch(OUT), CODES_AT = codec_codes_at(OUT);
    constexpr bool DECODED = (OUT & kCodeDecoded) != 0, CODES = (OUT & kCodeCodes) != 0;
    static_assert(DECODED || CODES, "an output at least");
    __shared__ __attribute__((aligned(16))) int region[kFilterLanes * PITCH];
    __shared__ __attribute__((aligned(16))) long long where[kFilterLanes][2];
    __shared__ int steps[kAdpcmSteps];
    const int lane = threadIdx.x;
    int* const mine = region + lane * PITCH;
    T* const staged = reinterpret_cast<T*>(mine);
    uint8_t* const stagedCodes = reinterpret_cast<uint8_t*>(mine + CODES_AT);
    const In* __restrict__ in = static_cast<const In*>(A.in);
    for (int i = lane; i < kAdpcmSteps; i += kFilterLanes) steps[i] = kAdpcmTable.step[i];
    for (long long g = blockIdx.x; g < A.nGroups; g += gridDim.x) {
        const FilterGroup G = A.groups[g];
        const StageLaneRow me = A.rows[G.first + lane];
        int* const kept = A.state + me.state * 2;                  // (a filler has no section and touches nothing)
        int val = me.sections ? kept[0] : 0, idx = me.sections ? kept[1] : 0;
        where[lane][0] = me.sections ? me.dst : -1;
        where[lane][1] = me.outLen;
        const long long width = A.rowStride > 0 ? A.rowStride : G.outMost;
        In next[kFilterLanes];
        filter_load_rows(next, in, me.src, me.len, 0, lane);
        bool zeroed = false;
        for (long long t0 = 0; t0 < width; t0 += TILE) {
            if (t0 < G.outMost) {
                __syncthreads();                                   // the tile before has left the region (and the step table is there)
#pragma unroll
                for (int q = 0; q < kFilterLanes; ++q) region[q * PITCH + lane] = codec_sample(next[q]);
                if (t0 + TILE < G.inMost) filter_load_rows(next, in, me.src, me.len, t0 + TILE, lane);
                else {
#pragma unroll
                    for (int q = 0; q < kFilterLanes; ++q) next[q] = (In)0;
                }
                __syncthreads();
                const long long live = me.outLen - t0;             // samples of the tile that are the lane's row's own; the rest is padding
                for (int t = 0; t < TILE; ++t) {
                    const bool on = t < live;                      // a step past the row's own count leaves val and idx as they are
                    int v = val, i = idx;
                    const int code = adpcm_encode(mine[t], steps[i], v, i);
                    val = on ? v : val;
                    idx = on ? i : idx;
                    if (DECODED) staged[t] = on ? codec_value<F32>(v) : (T)0;
                    if (CODES) stagedCodes[t] = on ? (uint8_t)code : (uint8_t)0;
                }
                __syncthreads();
            } else if (!zeroed) {                                  // (padded rows past the group's longest: +0 and code 0 without arithmetic)
                __syncthreads();
                for (int t = 0; t < PITCH; ++t) mine[t] = 0;
                zeroed = true;
                __syncthreads();
            }
            if (DECODED) codec_store_rows<T, PITCH, 0>(A.decoded, where, A.rowStride, t0, region, lane);
            if (CODES) codec_store_rows<uint8_t, PITCH, CODES_AT>(A.codes, where, A.rowStride, t0, region, lane);
        }
        if (me.sections) {
            kept[0] = me.ended ? 0 : val;
            kept[1] = me.ended ? 0 : idx;
        }
        __syncthreads();                                           // the last tile has left before the next group's first
    }
}

}  // namespace klatt
#endif
