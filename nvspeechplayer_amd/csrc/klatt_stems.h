// klatt_stems.h -- the signal stems of a set batch (speechPlayer_batch_exportStems).
//
// What every synthesis kernel computes on a sample and throws away: the voice and aspiration parts of the excitation, their sum (what
// enters the cascade), the frication (what enters the parallel bank), the outputs of the two filter branches and the mixed sample
// before it is clipped and truncated.  The definition is in include/speechPlayer_batch.h; it is dsp_sample<MODE_EXACT, true> of
// klatt_device.h with the seven values kept (stem_sample below), whatever the batch's mode, layout or plan.
//
//   klatt_stems   ONE WAVEFRONT per 64 export rows, one lane per row: the lane kernel's frame state machine (Lane, event_step,
//                 fade_update<MODE_EXACT, false, kNumRes>, frame_window, vib_live, the noise functions -- klatt_device.h, unchanged)
//                 around stem_sample, with the lane kernel's branch-free blocks of steady or fade samples wherever every live lane is
//                 inside such a stretch.  The noisy arithmetic runs for every row: for a row whose noise gains are all zero it gives
//                 the bits the quiet short cut gives.
//                 The output is PLANAR, [row][column][sample].  A lane stages the DISTINCT columns asked for, already converted to
//                 the output's element type, in its row of an LDS tile of T samples ([lane][slot][sample], the row padded by 8 bytes:
//                 an odd number of 8-byte words, so that the lanes' ds_write_b64 fall on different banks).  After T samples the
//                 wavefront writes the tile out: per requested column (a repeated column is stored again from the same slot), lane =
//                 (row, 16-byte piece), consecutive lanes on consecutive pieces of one (row, column) segment -- whole 64- or
//                 128-byte segments, as flush_tile writes PCM.  A piece that is not 16-byte aligned in the caller's buffer (packed rows
//                 of odd length, a buffer aligned to the element only) or that holds an utterance's last, partial elements goes out
//                 element by element.  Past an utterance's end a padded row is zeroed by the same wavefront when its rows are done.
//                 T = 16 while the staged columns take at most 32 bytes per sample (float32: always; float64: up to four columns), else
//                 8 (float64, five to seven columns; the blocks are then 8 samples long): with oldP / newP (45 KB) a workgroup
//                 stays below 80 KiB, two to a CU.
//                 The host hands the rows over sorted by length (a wavefront runs as long as its longest lane); a row carries its own
//                 place in the output.
#pragma once

#include <stdint.h>

#include "klatt_device.h"

namespace klatt {

constexpr int kStemVoice = 0, kStemAspiration = 1, kStemSource = 2, kStemFrication = 3, kStemCascade = 4, kStemParallel = 5, kStemOutput = 6;
constexpr int kStemColumns = 7;             // SPEECHPLAYER_STEM_COLUMNS
constexpr int kStemTilePad = 8;             // bytes after a lane's tile row
constexpr int kStemLdsBudget = 80 * 1024;

struct StemRow {             // 32 B per export row
    long long frame0;        // first frame of the utterance's list
    long long out;           // the row's first element in the output
    uint32_t nFrames;
    uint32_t seed;
    uint32_t length;         // L
    uint32_t pad;
};
static_assert(sizeof(StemRow) == 32, "StemRow layout");

struct StemArgs {
    KernelArgs K;                    // frames, meta words and the sample-rate constants (nothing else is read)
    const StemRow* rows;             // longest first
    long long nRows;
    const int* columns;              // [nColumns] as asked for
    int nColumns;
    int nSlots;                      // distinct columns asked for
    int slotOf[kStemColumns];        // the tile slot of column c; -1: not asked for
    long long rowStride;             // 0: packed (a row's columns are L apart)
    void* out;
};

// samples per tile for nSlots staged columns of elSize bytes
__host__ __device__ constexpr int stem_tile(int nSlots, int elSize) { return nSlots * elSize <= 32 ? 16 : 8; }
// bytes of a lane's tile row, pad included
__host__ __device__ constexpr int stem_tile_stride(int nSlots, int elSize) { return nSlots * stem_tile(nSlots, elSize) * elSize + kStemTilePad; }
// dynamic LDS of a workgroup: oldP, newP | tile | rowOut[64] i64 | rowLen[64], rowFull[64] u32
__host__ __device__ constexpr int stem_lds_bytes(int nSlots, int elSize) { return 2 * kSlots * kLanes * 8 + kLanes * stem_tile_stride(nSlots, elSize) + kLanes * 16; }
static_assert(stem_lds_bytes(kStemColumns, 8) <= kStemLdsBudget && stem_lds_bytes(4, 8) <= kStemLdsBudget && stem_lds_bytes(kStemColumns, 4) <= kStemLdsBudget,
              "two workgroups to a CU");

// ---- one sample from the lane's current parameters: dsp_sample<MODE_EXACT, true> (reference src/speechWaveGenerator.cpp:72-86, :147-180,
// :203-208) with its intermediate values kept in v[kStemColumns].  Every operation is rounded on its own (-ffp-contract=off).
__device__ __forceinline__ void stem_sample(Lane& s, const KernelArgs& A, uint32_t ninc, bool waveVib, double* v)
{
    double vib = 1.0;
    if (waveVib) {   // wave-uniform
        const double vs = s.cur[2];
        const double adv = frac_toward_zero(div_by(vs, A.sampleRateF, A.invSampleRate) + s.vibPhase);
        s.vibPhase = (vs != 0.0) ? adv : s.vibPhase;
        vib = (sin(s.vibPhase * 6.283185307179586) * 0.06 * s.cur[1]) + 1.0;
    }
    s.pitchPhase = frac_toward_zero(div_by(s.cur[0] * vib, A.sampleRateF, A.invSampleRate) + s.pitchPhase);
    double voice = (s.pitchPhase * 2.0) - 1.0;
    s.aspNoise = noise_uniform(s.noiseState) + 0.75 * s.aspNoise;            // :40
    double asp = s.aspNoise * 0.2;
    double turb = asp * s.cur[3];
    turb = (s.pitchPhase >= s.cur[4]) ? turb : turb * 0.01;                   // glottis closed
    voice += turb;
    voice *= s.cur[5];
    asp *= s.cur[6];
    const double src = asp + voice;
    v[kStemVoice] = voice; v[kStemAspiration] = asp; v[kStemSource] = src;

    // cascade (:147-158): N0 anti-resonator (memory takes the INPUT, :133), NP mixed in by caNP, r6..r1
    const double x = (src * s.cur[44]) * 0.5;
    double o;
    {
        const double n0 = dot3<MODE_EXACT>(s.ra[0], x, s.rb[0], s.z1[0], s.rc[0], s.z2[0]);
        s.z2[0] = s.z1[0]; s.z1[0] = x;
        const double np = dot3<MODE_EXACT>(s.ra[1], n0, s.rb[1], s.z1[1], s.rc[1], s.z2[1]);
        s.z2[1] = s.z1[1]; s.z1[1] = np;
        o = fade_value(x, np, s.cur[23]);
    }
#pragma unroll
    for (int r = 2; r < 8; ++r) {
        const double y = dot3<MODE_EXACT>(s.ra[r], o, s.rb[r], s.z1[r], s.rc[r], s.z2[r]);
        s.z2[r] = s.z1[r]; s.z1[r] = y;
        o = y;
    }
    v[kStemCascade] = o;

    // frication + parallel bank (:205-206, :170-180)
    s.fricNoise = noise_uniform(noise_step(s.noiseState, ninc)) + 0.75 * s.fricNoise;
    s.noiseState = noise_step2(s.noiseState, noise_inc2(ninc));
    const double fric = s.fricNoise * 0.3 * s.cur[24];
    v[kStemFrication] = fric;
    const double y = (fric * s.cur[44]) * 0.5;
    double par = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int r = 8 + k;
        const double w = dot3<MODE_EXACT>(s.ra[r], y, s.rb[r], s.z1[r], s.rc[r], s.z2[r]);
        s.z2[r] = s.z1[r]; s.z1[r] = w;
        par += (w - y) * s.cur[37 + k];
    }
    par = fade_value(par, y, s.cur[43]);
    v[kStemParallel] = par;
    v[kStemOutput] = ((o + par) * s.cur[45]) * 4000.0;
}

typedef uint32_t StemU32x4 __attribute__((ext_vector_type(4)));

// n elements of zeros from p on, by the wavefront: 16-byte stores between the first and the last 16-byte boundary
template <typename E>
__device__ __forceinline__ void stem_zero_span(E* p, long long n, int lane)
{
    constexpr int EL = 16 / (int)sizeof(E);
    if (n <= 0) return;
    const long long toBoundary = (long long)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(E));
    const long long head = toBoundary < n ? toBoundary : n;
    if (lane < head) p[lane] = (E)0;
    const long long body = (n - head) / EL;
    StemU32x4* q = reinterpret_cast<StemU32x4*>(p + head);
    for (long long k = lane; k < body; k += kLanes) __builtin_nontemporal_store(StemU32x4{0u, 0u, 0u, 0u}, q + k);
    const long long done = head + body * EL;
    if (lane < n - done) p[done + lane] = (E)0;
}

template <bool F32, int T>
__global__ void __launch_bounds__(kLanes) klatt_stems(const StemArgs SA)
{
    typedef typename std::conditional<F32, float, double>::type E;
    constexpr int EL = 16 / (int)sizeof(E);                 // elements per 16-byte piece
    constexpr int kPieces = T / EL;                         // pieces per (row, column) segment of a tile
    constexpr int kRowsPerPass = kLanes / kPieces;
    constexpr int BL = T < kBlock ? T : kBlock;             // samples per specialised block
    const KernelArgs& A = SA.K;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* const oldP = reinterpret_cast<double*>(lds);
    double* const newP = oldP + kSlots * kLanes;
    unsigned char* const tile = lds + 2 * kSlots * kLanes * 8;
    const int tileStride = SA.nSlots * T * (int)sizeof(E) + kStemTilePad;
    long long* const rowOut = reinterpret_cast<long long*>(tile + kLanes * tileStride);
    uint32_t* const rowLen = reinterpret_cast<uint32_t*>(rowOut + kLanes);      // samples a row has staged or written so far
    uint32_t* const rowFull = rowLen + kLanes;                                   // its utterance's length

    const int lane = threadIdx.x;
    const long long slot = (long long)blockIdx.x * kLanes + lane;
    const bool live = slot < SA.nRows;
    StemRow row;
    row.frame0 = 0; row.out = -1; row.nFrames = 0; row.seed = 0; row.length = 0; row.pad = 0;
    if (live) row = SA.rows[slot];
    UttDesc d;
    d.frameStart = row.frame0; d.outStart = 0; d.nFrames = row.nFrames; d.seed = row.seed; d.flags = 0; d.length = row.length;
    const FrameWindow w = frame_window(A, d);
    const double* const myFrames = A.frames + w.base * kNumParams;
    const FrameMeta* const myMeta = A.meta + w.base;
    const uint32_t nkey = noise_key(d.seed), ninc = noise_inc(d.seed);

    // ---- fresh-handle state, as klatt_synthesize
    Lane s;
#pragma unroll
    for (int i = 0; i < kNumParams; ++i) s.cur[i] = 0.0;
    s.old0 = 0.0; s.new0 = 0.0; s.oldInc = 0.0; s.newInc = 0.0; s.invFade = 1.0;
    s.cnt = 0; s.oldMin = 0; s.newMin = 0; s.newFade = 1;
    s.hasNew = false; s.oldNull = true; s.newNull = false;
    s.lastIndex = -1; s.resMask = 0; s.nextFrame = 0; s.noiseState = noise_first(nkey, ninc); s.produced = 0;
    s.done = !live; s.drained = false; s.vibFrames = false;
#pragma unroll
    for (int r = 0; r < kNumRes; ++r) { s.ra[r] = 0.0; s.rb[r] = 2.0; s.rc[r] = -1.0; s.z1[r] = 0.0; s.z2[r] = 0.0; }
    s.pitchPhase = 0.0; s.vibPhase = 0.0; s.aspNoise = 0.0; s.fricNoise = 0.0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) { oldP[k * kLanes + lane] = 0.0; newP[k * kLanes + lane] = 0.0; }

    rowOut[lane] = row.out;
    rowLen[lane] = 0;
    rowFull[lane] = row.length;
    __syncthreads();

    E* const myRow = reinterpret_cast<E*>(tile + lane * tileStride);
    uint32_t it = 0;    // wave-uniform: samples stepped (every live lane emits one per step until it is done)

    auto keep = [&](const double* v, uint32_t pos) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < kStemColumns; ++c) {
            const int sl = SA.slotOf[c];      // wave-uniform
            if (sl >= 0) myRow[sl * T + pos] = (E)v[c];
        }
    };

    // write the tile out: per requested column, lane -> (row, 16-byte piece), kPieces consecutive lanes per (row, column) segment
    auto flush_tile = [&](uint32_t tileStart) __attribute__((always_inline)) {
        rowLen[lane] = min(s.produced, d.length);
        __syncthreads();
        for (int q = 0; q < SA.nColumns; ++q) {
            const int sl = SA.slotOf[SA.columns[q]];
#pragma unroll
            for (int p = 0; p < kPieces; ++p) {
                const int r = p * kRowsPerPass + lane / kPieces;
                const int piece = lane % kPieces;
                const uint32_t first = tileStart + (uint32_t)(piece * EL);
                const uint32_t len = rowLen[r];
                const long long base = rowOut[r];
                if (base >= 0 && len > first) {
                    const unsigned char* src = tile + r * tileStride + (sl * T + piece * EL) * (int)sizeof(E);
                    const uint32_t nEl = min(len - first, (uint32_t)EL);
                    const long long colStride = SA.rowStride ? SA.rowStride : (long long)rowFull[r];      // (a packed row's columns are its length apart)
                    E* dst = static_cast<E*>(SA.out) + base + (long long)q * colStride + first;
                    if (nEl == (uint32_t)EL && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                        const uint2 lo = reinterpret_cast<const uint2*>(src)[0], hi = reinterpret_cast<const uint2*>(src)[1];
                        __builtin_nontemporal_store(StemU32x4{lo.x, lo.y, hi.x, hi.y}, reinterpret_cast<StemU32x4*>(dst));
                    } else {
                        const E* e = reinterpret_cast<const E*>(src);
#pragma unroll
                        for (int i = 0; i < EL; ++i) if ((uint32_t)i < nEl) dst[i] = e[i];
                    }
                }
            }
        }
        __syncthreads();
    };

    // one general step: per lane an event, fade or steady sample
    auto general_step = [&]() __attribute__((always_inline)) {
        bool emit = false;
        if (!s.done) {
            s.cnt++;
            const bool fading = s.hasNew && s.cnt <= s.newFade;
            const bool steady = !s.hasNew && s.cnt <= s.oldMin;
            if (fading) {
                fade_update<MODE_EXACT, false, kNumRes>(s, A, oldP, newP, nullptr, lane);
                emit = true;
            } else if (steady) {
                s.cur[0] += s.oldInc;          // glide the pitch (reference src/frame.cpp:76-79)
                s.old0 = s.cur[0];
                emit = true;
            } else {
                emit = event_step(s, d, myFrames, myMeta, w.off, w.mask, oldP, newP, lane);
            }
        }
        const bool waveVib = __any(emit && vib_live(s));
        if (emit) {
            double v[kStemColumns];
            stem_sample(s, A, ninc, waveVib, v);
            keep(v, it % T);
            s.produced++;
        }
        it++;
    };

    // BL branch-free samples; KIND 0 = every live lane steady, 1 = every live lane fading
    auto block_run = [&](auto kindTag) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kindTag)::value;
        const uint32_t tpos = it % T;
        if (!s.done) {
#pragma nounroll
            for (int i = 0; i < BL; ++i) {
                s.cnt++;
                if (KIND == 0) { s.cur[0] += s.oldInc; s.old0 = s.cur[0]; }
                else fade_update<MODE_EXACT, false, kNumRes>(s, A, oldP, newP, nullptr, lane);
                double v[kStemColumns];
                stem_sample(s, A, ninc, false, v);
                keep(v, tpos + i);
            }
            s.produced += BL;
        }
        it += BL;
    };

    while (true) {
        if (!__any(!s.done)) break;
        // samples left in the lane's current stretch (0 = the next sample is an event)
        const uint32_t rem = s.hasNew ? (s.newFade - s.cnt) : (s.oldMin > s.cnt ? s.oldMin - s.cnt : 0u);
        const bool roomy = s.done || rem >= (uint32_t)BL;
        const bool fits = (it % T) + BL <= (uint32_t)T;
        int kind = -1;
        if (fits && __all(roomy) && !__any(!s.done && vib_live(s))) {
            if (!__any(!s.done && s.hasNew)) kind = 0;
            else if (!__any(!s.done && !s.hasNew)) kind = 1;
        }
        if (kind == 0) block_run(std::integral_constant<int, 0>());
        else if (kind == 1) block_run(std::integral_constant<int, 1>());
        else general_step();
        if ((it % T) == 0) flush_tile(it - T);
    }
    if ((it % T) != 0) flush_tile(it - (it % T));

    // a padded row is zero past its utterance's end
    if (SA.rowStride) {
        for (int r = 0; r < kLanes; ++r) {
            const long long base = rowOut[r];
            if (base < 0) continue;
            const long long len = (long long)rowFull[r];
            for (int q = 0; q < SA.nColumns; ++q)
                stem_zero_span(static_cast<E*>(SA.out) + base + (long long)q * SA.rowStride + len, SA.rowStride - len, lane);
        }
    }
}

}  // namespace klatt
