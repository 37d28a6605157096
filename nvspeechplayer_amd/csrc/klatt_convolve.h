// klatt_convolve.h -- a batch's PCM convolved with impulse responses (speechPlayer_batch_exportConvolved) and plain PCM convolved on the
// host (speechPlayer_pcmConvolve).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_RES_HD are
// compiled for the host and for the device from the same source: the input conversion (res_input of klatt_resample.h), the step
// acc = fmaf(x, h, acc) -- ONE correctly rounded binary32 fused multiply-add, written __builtin_fmaf so that it is fused whatever the
// contraction flag says and exact on the host whatever the build flags -- the closing acc + 0.0f and the int16 conversion (res_int16).
//
//   The plan        conv_plan: the responses back to back with their starts, and the refusals (messages without the entry point's prefix).
//   The statement   convolve_host: for every output m, acc = +0, then k = 0 .. K-1 ascending acc = conv_step(acc, x[m - k], h[k]) with
//                   x = +0 outside 0 .. L-1, then conv_finish.
//   The lemma       For finite operands, inserting or removing terms whose product is +-0 -- samples outside the utterance, zero taps,
//                   the zero padding of a tap block -- does not change y[m]: a +-0 product added to a nonzero acc returns acc, added to a
//                   zero acc returns a zero; a zero acc of either sign followed by a nonzero product p returns RN(p).  Two such sequences
//                   agree at every step except possibly in the sign of a zero, and conv_finish's + 0.0f makes that +0.
//   The indices     What the kernel visits, as plain functions a stand-alone program checks against brute force
//                   (tests/native/check_convolve.cpp): conv_blocks, conv_block_taps, conv_block_padded, conv_block_skipped, conv_block_last,
//                   conv_staged_sample, conv_window.
//   conv_rows       The one body of klatt_convolve and of klatt_stage_convolve (klatt_stage_window.h: the convolution fed chunk by chunk), its
//                   two entry points; KEPT is the compile-time switch for "this launch carries state", and the entry point hands in the reader.
//   klatt_convolve  A 256-lane workgroup takes tiles of kConvolveTile consecutive outputs of one row; lane l owns the FOUR outputs
//                   4 l .. 4 l + 3 of the tile and keeps their sums in registers across the tap blocks, which is what keeps every
//                   output's terms in ascending k from the first block to the last.  Per block of kConvolveBlock taps the workgroup stages
//                   the taps in LDS (padded with +0 to a multiple of four) and the tile's inputs for them REVERSED:
//                   xr[p] = x[t0 + T - kb - p], masked to 0 <= n < L and converted by the reader (klatt_tiles.h: tile_read downwards from
//                   conv_read_first, from int16 or float32), each loaded once.  Output o, tap
//                   kb + q reads xr[(T - o) + q]: both the taps and the inputs are walked upwards.  A step takes four taps: one
//                   16-byte LDS read of the taps at the same address in every lane (a broadcast), one 16-byte read of four new inputs at
//                   a lane stride of 16 bytes (conflict-free: the 16 lanes of a ds_read_b128 group cover 64 distinct banks), a sliding
//                   window of seven inputs in registers, and sixteen conv_step (conv_step4), which the compiler pairs into eight
//                   v_pk_fma_f32.  A block whose inputs lie wholly outside 0 .. L-1 is skipped (the lemma).  The tiles are walked and
//                   the values written as klatt_tiles.h says, a padded row's remainder as +0.  LDS: 4 KB of taps + 8 KB of inputs
//                   (reused for the staged values) = 12 KB.
#pragma once

#include "klatt_resample.h"

namespace klatt {

constexpr int kConvolveTile = 1024;                  // consecutive outputs of one row a workgroup takes at a time (4 per lane)
constexpr int kConvolveBlock = 1024;                 // taps staged in LDS at a time (a multiple of 4)
constexpr int kConvolveMaxTaps = 65536;              // of one response
constexpr long long kConvolveMaxTable = 1ll << 20;   // taps of all responses of a call (4 MB: the staging block has no lower limit)
constexpr float kConvolveMaxTap = 4294967296.0f;     // |h[k]| <= 2^32: with K <= 2^16 and |x| <= 32768 / 32767 no sum overflows

static_assert(kConvolveTile == 4 * 256 && kConvolveBlock % 4 == 0 && kConvolveBlock >= 4, "four outputs per lane, four taps per step");

// One term: acc + x h, rounded once
KLATT_RES_HD float conv_step(float acc, float x, float h) { return __builtin_fmaf(x, h, acc); }

// The closing + 0.0f: a zero of either sign becomes +0
KLATT_RES_HD float conv_finish(float acc) { return acc + 0.0f; }

// Four taps h[0 .. 3] (taps q .. q + 3 of a block) of a lane's four outputs: output j (o = 4 l + j) takes v[t + 3 - j] against h[t],
// t ascending, where v[0 .. 6] = xr[w + q + 1 .. w + q + 7] and w = conv_window(l): the last three of the step before and four new
KLATT_RES_HD void conv_step4(float (&acc)[4], const float (&v)[7], const float (&h)[4])
{
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 4; ++j) acc[j] = conv_step(acc[j], v[t + 3 - j], h[t]);
    }
}

// A lane's four finished sums, outputs o0 .. o0 + 3 of the tile, staged in the output's type: +0 past the `live` outputs
template <bool F32> KLATT_RES_HD void conv_stage4(TileValue<F32>* staged, const float (&acc)[4], int o0, int live)
{
    for (int q = 0; q < 4; ++q) staged[o0 + q] = o0 + q < live ? res_value<F32>(conv_finish(acc[q])) : (TileValue<F32>)0;
}

// ---- the kernel's index arithmetic ---------------------------------------------------------------------------------------------------------
inline int conv_blocks(long long K) { return (int)((K + kConvolveBlock - 1) / kConvolveBlock); }
// Block b holds taps kb = b kConvolveBlock .. kb + conv_block_taps - 1, staged as conv_block_padded values (+0 past the taps)
KLATT_RES_HD int conv_block_taps(int K, int kb) { return K - kb < kConvolveBlock ? K - kb : kConvolveBlock; }
KLATT_RES_HD int conv_block_padded(int taps) { return (taps + 3) & ~3; }
// The outputs t0 .. t0 + live - 1 (live >= 1) against taps kb .. kb + taps - 1 read inputs t0 - kb - taps + 1 .. t0 + live - 1 - kb.
// conv_block_last: they all lie below 0, and so do those of every later block.  conv_block_skipped: they all lie outside 0 .. L-1.
KLATT_RES_HD bool conv_block_last(long long t0, int live, int kb) { return t0 + live - 1 - kb < 0; }
KLATT_RES_HD bool conv_block_skipped(long long t0, int live, long long L, int kb, int taps)
{
    return conv_block_last(t0, live, kb) || t0 - kb - (taps - 1) >= L;
}
// xr[p] of the tile at t0 and the block at kb holds input sample conv_staged_sample (p = 0 .. kConvolveTile + padded - 1)
KLATT_RES_HD long long conv_staged_sample(long long t0, int kb, int p) { return t0 + kConvolveTile - kb - p; }
// ... which is the reader's run downwards from conv_read_first
KLATT_RES_HD long long conv_read_first(long long t0, int kb) { return t0 + kConvolveTile - kb; }
// Lane l reads the aligned four values xr[conv_window(l) + q + 4 .. + 7] for taps q .. q + 3 (and xr[conv_window(l) .. + 3] first)
KLATT_RES_HD int conv_window(int lane) { return kConvolveTile - 4 - 4 * lane; }

// ---- the request, as every entry point plans it on the host -----------------------------------------------------------------------------
struct ConvPlan {
    long long nIr = 0;
    std::vector<long long> start;      // [nIr + 1]
    std::vector<float> taps;           // the responses back to back
    long long most = 0;                // the longest response
};

// The plan of a request, or false with `why` set (without the entry point's prefix).  irOf (nRows entries; may be null) is checked by
// conv_row, row by row.
inline bool conv_plan(ConvPlan& P, const float* ir, const long long* irStart, long long nIr, int tail, std::string& why)
{
    char buf[200];
    if (tail != 0 && tail != 1) { snprintf(buf, sizeof buf, "tail %d (0 the first L outputs, 1 the full convolution)", tail); why = buf; return false; }
    if (nIr < 1) { snprintf(buf, sizeof buf, "%lld impulse responses (at least 1)", nIr); why = buf; return false; }
    if (!ir || !irStart) { why = "no impulse responses (ir and irStart)"; return false; }
    if (irStart[0] != 0) { snprintf(buf, sizeof buf, "irStart[0] = %lld (the first response starts at 0)", irStart[0]); why = buf; return false; }
    long long most = 0;
    for (long long j = 0; j < nIr; ++j) {
        const long long a = irStart[j], b = irStart[j + 1];
        if (b <= a) { snprintf(buf, sizeof buf, "irStart[%lld] = %lld is not above irStart[%lld] = %lld (a response has at least 1 tap)", j + 1, b, j, a); why = buf; return false; }
        if (b - a > kConvolveMaxTaps) { snprintf(buf, sizeof buf, "response %lld has %lld taps (at most %d)", j, b - a, kConvolveMaxTaps); why = buf; return false; }
        if (b > kConvolveMaxTable) { snprintf(buf, sizeof buf, "the responses have more than %lld taps in all", kConvolveMaxTable); why = buf; return false; }
        most = b - a > most ? b - a : most;
    }
    for (long long j = 0; j < nIr; ++j)
        for (long long k = irStart[j]; k < irStart[j + 1]; ++k)
            if (!(fabsf(ir[k]) <= kConvolveMaxTap)) {      // (a NaN fails the comparison)
                snprintf(buf, sizeof buf, "tap %lld of response %lld is %g (finite, at most 2^32 in magnitude)", k - irStart[j], j, (double)ir[k]);
                why = buf; return false;
            }
    P.nIr = nIr; P.most = most;
    P.start.assign(irStart, irStart + nIr + 1);
    P.taps.assign(ir, ir + irStart[nIr]);
    return true;
}

// The response of row i, or -1 with `why` set
inline long long conv_row(const ConvPlan& P, const long long* irOf, long long i, std::string& why)
{
    char buf[200];
    if (!irOf) {
        if (P.nIr == 1) return 0;
        snprintf(buf, sizeof buf, "no irOf with %lld impulse responses (NULL takes exactly 1)", P.nIr); why = buf; return -1;
    }
    if (irOf[i] < 0 || irOf[i] >= P.nIr) { snprintf(buf, sizeof buf, "irOf[%lld] = %lld is not a response (%lld)", i, irOf[i], P.nIr); why = buf; return -1; }
    return irOf[i];
}

inline long long conv_length(long long L, long long K, int tail) { return tail ? L + K - 1 : L; }

// ---- the host's statement (speechPlayer_pcmConvolve): the shared functions in a plain loop ------------------------------------------------
// format 1: out is float[Lout]; format 0: int16_t[Lout].  Returns Lout.  In: int16_t (PCM) or float (a signal's samples).
template <typename In>
inline long long convolve_host(const In* pcm, long long length, const float* h, long long K, int tail, int format, void* out)
{
    const long long Lout = conv_length(length, K, tail);
    // x[n] for n = -(K-1) .. length-1, +0 outside the signal: xp[n + K - 1]
    std::vector<float> xp((size_t)(length + K - 1) + (size_t)(tail ? K - 1 : 0), 0.0f);
    for (long long n = 0; n < length; ++n) xp[(size_t)(n + K - 1)] = tile_x(pcm[n]);
    for (long long m = 0; m < Lout; ++m) {
        const float* x = xp.data() + (m + K - 1);      // x[-k] is x[m - k]
        float acc = 0.0f;
        for (long long k = 0; k < K; ++k) acc = conv_step(acc, x[-k], h[k]);
        res_store(out, format, m, conv_finish(acc));
    }
    return Lout;
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

// first element and samples of a row's input (the pool's utterance, a signal's row); its outputs; its first element in the output; its response's first tap and its taps
struct ConvRow { long long src, len, outLen, dst, irAt, taps; };

struct ConvArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const ConvRow* rows;
    TileOut tile;
    const float* taps;                   // the responses back to back
};

// The one body of klatt_convolve and of klatt_stage_convolve (klatt_stage_window.h), its two entry points.  KEPT: the launch carries state --
// output t of a row is y[N + t] of the row's stream, whose samples 0 .. N + len - 1 exist (the block tests run at that index), its taps
// are the row's history + 1, and `read` fills the reversed inputs from the virtual row; otherwise from the row itself (tile_read).
template <bool KEPT, bool F32, typename In, class Args, class Read>
__device__ __forceinline__ void conv_rows(const Args& A, Read read)
{
    using T = TileValue<F32>;
    constexpr int TILE = kConvolveTile;
    __shared__ __attribute__((aligned(16))) float hs[kConvolveBlock];
    __shared__ __attribute__((aligned(16))) float xr[kConvolveTile + kConvolveBlock];
    T* staged = reinterpret_cast<T*>(xr);      // (behind a barrier: the last block's reads are done)
    const int tid = threadIdx.x;
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, TILE, r, t0);
        const auto row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.outLen, t0, TILE);
        const int live = tile_live(n, row.outLen, t0);      // outputs of the tile inside the row; the rest is padding
        const In* __restrict__ pcm = static_cast<const In*>(A.in) + row.src;
        const float* __restrict__ h = A.taps + row.irAt;
        long long first = t0, L = row.len;                   // the tile's first output and the samples there are, in the coordinates of the block tests
        int K;
        if constexpr (KEPT) { first = row.N + t0; L = row.N + row.len; K = (int)row.H + 1; }
        else K = (int)row.taps;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live > 0) {
            for (int kb = 0; kb < K; kb += kConvolveBlock) {      // (every condition here is uniform over the workgroup)
                if (conv_block_last(first, live, kb)) break;
                const int taps = conv_block_taps(K, kb), padded = conv_block_padded(taps);
                if (conv_block_skipped(first, live, L, kb, taps)) continue;
                __syncthreads();                                  // the block before has been read
                for (int i = tid; i < padded; i += 256) hs[i] = i < taps ? h[kb + i] : 0.0f;
                read(xr, pcm, row, conv_read_first(first, kb), TILE + padded, tid);
                __syncthreads();
                const float4* __restrict__ xw = reinterpret_cast<const float4*>(xr + conv_window(tid));
                const float4* __restrict__ hw = reinterpret_cast<const float4*>(hs);
                float4 a = xw[0];
                const int steps = padded >> 2;
                for (int q = 0; q < steps; ++q) {
                    const float4 b = xw[q + 1], hq = hw[q];
                    const float v[7] = {a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    const float h4[4] = {hq.x, hq.y, hq.z, hq.w};
                    conv_step4(acc, v, h4);
                    a = b;
                }
            }
        }
        __syncthreads();
        conv_stage4<F32>(staged, acc, 4 * tid, live);
        __syncthreads();
        tile_store<T>(A.tile.out, row.dst + t0, n, staged, tid);
        __syncthreads();      // `staged` is the next tile's xr
    }
}

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_convolve(const ConvArgs A)
{
    conv_rows<false, F32, In>(A, [](float* xr, const In* __restrict__ pcm, const ConvRow& row, long long s0, int count, int tid) {
        tile_read<-1>(xr, pcm, row.len, s0, count, tid);
    });
}

}  // namespace klatt
#endif
