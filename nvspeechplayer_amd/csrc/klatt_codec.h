// klatt_codec.h -- a batch's PCM through the G.711 laws and the IMA/DVI ADPCM codec (speechPlayer_batch_exportCoded) and plain PCM coded
// on the host (speechPlayer_pcmCode, speechPlayer_codecDecode).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_RES_HD are
// compiled for the host and for the device from the same source: the input conversion (codec_sample: an int16 as it is, a float32 through
// res_int16 of klatt_resample.h), the two laws' encoders and decoders, one ADPCM sample (adpcm_encode, adpcm_apply) and the output
// conversion (codec_value: the decoded int16, or tile_x of it).  All arithmetic is int32; >> of a negative value is arithmetic (two's
// complement, as every compiler this project builds with has it); codec_top is the bit index of the highest set bit.
//
//   The statement   code_host: per sample s = codec_sample(x[n]); G.711: code = encode(s), d = decode(code); ADPCM: the recursion from
//                   val = 0, idx = 0 at a row's first sample, d = val.  One code per sample, a uint8 (0 .. 255, ADPCM 0 .. 15); row
//                   lengths unchanged.  decode_host is the decoder alone, for ADPCM adpcm_apply driven by the codes: it rebuilds the
//                   encoder's val, which is why the encoder gives d without a second pass.
//   klatt_code_g711 The tile walk of klatt_tiles.h: a 256-lane workgroup per tile of kCodeTile samples of one row (tile_locate).  A
//                   sample is read masked to the row (nothing outside a row is loaded: a lane past the row's end loads the row's last sample
//                   again, so that a tile's loads are issued together without a branch, and takes +0 and code 0), encoded and decoded by the arithmetic above -- no
//                   table, codec_top is one v_ffbh_u32 --, and staged in LDS in the output's type at the offset its first element has in its
//                   aligned 16 bytes of the output (codec_lead), so that a lane's block is one aligned 16-byte LDS read and one 16-byte
//                   store (codec_store_block; kTileLane<uint8_t> is 16: the codes leave in 16-byte stores as well; the run's two ends go
//                   element by element, as tile_store_lane's).  A padded row's tiles past its end are +0 and code 0 without loads or
//                   arithmetic.  2 or 4 bytes in, 1 to 5 out, some 20 integer operations a sample.
//   klatt_code_adpcm
//                   The recursion is sequential along time and parallel across rows only, so it takes klatt_filter's scheme whole: one
//                   wavefront per group of 64 rows (filter_pack with one section a row: one bucket, rows by length descending), a lane per
//                   row, val and idx in two registers from the first sample to the last.  Time is walked in tiles of kFilterTile samples:
//                   filter_load_rows' masked loads, issued a tile ahead and waiting in registers during the steps; the samples written as
//                   int32 (codec_sample) into the wavefront's LDS region at an odd dword pitch, so lane r reads element [r][t] without
//                   bank conflicts; the outputs staged IN PLACE in the output's type (an element is at most as wide as the int32 it
//                   replaces, and element t is read before it is written); both outputs: the codes get a run of their own behind the
//                   row's 64 dwords, at a wider pitch, kept odd.  The staged runs leave through codec_store_rows: tile_store_lane with 32
//                   (float32), 16 (int16) or 8 (uint8: 64 codes touch at most 5 aligned 16 bytes) lanes a row.  The step table is 89
//                   dwords of LDS read per lane by idx -- a lane-indexed register array would become scratch.
//   Out of scope    G.722, G.726, GSM and anything without an independent statement to hold it to; packed nibbles (codes[0::2] << 4 |
//                   codes[1::2] is the usual byte order) and WAV block headers or predictor resets; packet loss; live handles through these
//                   kernels (the ADPCM state would have to persist across pulls: klatt_stage.h keeps it); NodePlayer.
#pragma once

#include "klatt_filter.h"

namespace klatt {

constexpr int kCodecUlaw = 0, kCodecAlaw = 1, kCodecAdpcm = 2, kCodecCount = 3;
constexpr int kCodeTile = 1024;                      // consecutive samples of one row a workgroup of klatt_code_g711 takes at a time
constexpr int kAdpcmSteps = 89;
constexpr int kCodecPitchBoth = kFilterPitch + kFilterTile / 4;      // dwords between rows when the codes have a run of their own: 81
static_assert(kFilterPitch % 2 == 1 && kCodecPitchBoth % 2 == 1, "odd pitches: lane r's element t lies in bank (r pitch + t) mod 64, distinct across lanes");

// The IMA step table
struct AdpcmTable { int step[kAdpcmSteps]; };
constexpr AdpcmTable kAdpcmTable{{
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963,
    1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358,
    5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623,
    27086, 29794, 32767}};

// The bit index of v's highest set bit, v > 0
KLATT_RES_HD int codec_top(int v) { return 31 - __builtin_clz((unsigned)v); }

// The int16 sample every codec takes: a row's int16 itself, a float32 clipped and rounded to nearest even (res_int16(tile_x(s)) == s)
KLATT_RES_HD int codec_sample(int16_t s) { return (int)s; }
KLATT_RES_HD int codec_sample(float x) { return (int)res_int16(x); }
// A decoded sample in the output's type: format 0 itself, format 1 tile_x of it
template <bool F32> KLATT_RES_HD TileValue<F32> codec_value(int d) { if (F32) return (TileValue<F32>)tile_x(d); return (TileValue<F32>)d; }

// ---- G.711 --------------------------------------------------------------------------------------------------------------------------------
KLATT_RES_HD int ulaw_encode(int s)
{
    int v = s >> 2, m = 0xFF;
    if (v < 0) { v = -v; m = 0x7F; }
    if (v > 8158) v = 8158;                // (audioop clips at 8159 and gives the one sum that then reaches 8192 the top code: the same codes)
    v += 33;
    const int seg = codec_top(v) - 5;      // 0 .. 7: v is 33 .. 8191
    return ((seg << 4) | ((v >> (seg + 1)) & 15)) ^ m;
}
KLATT_RES_HD int ulaw_decode(int code)
{
    const int c = ~code & 255, t = (((c & 15) << 3) + 132) << ((c & 0x70) >> 4);
    return (c & 0x80) ? 132 - t : t - 132;
}
KLATT_RES_HD int alaw_encode(int s)
{
    int v = s >> 3, m = 0xD5;
    if (v < 0) { m = 0x55; v = -v - 1; }
    const int seg = v < 32 ? 0 : codec_top(v) - 4;      // 0 .. 7: v is 0 .. 4095
    return ((seg << 4) | (seg < 2 ? (v >> 1) & 15 : (v >> seg) & 15)) ^ m;
}
KLATT_RES_HD int alaw_decode(int code)
{
    const int c = code ^ 0x55, seg = (c & 0x70) >> 4;
    int t = (c & 15) << 4;
    if (seg == 0) t += 8;
    else if (seg == 1) t += 0x108;
    else t = (t + 0x108) << (seg - 1);
    return (c & 0x80) ? t : -t;
}
template <int LAW> KLATT_RES_HD int g711_encode(int s) { return LAW == kCodecUlaw ? ulaw_encode(s) : alaw_encode(s); }
template <int LAW> KLATT_RES_HD int g711_decode(int code) { return LAW == kCodecUlaw ? ulaw_decode(code) : alaw_decode(code); }

// ---- IMA/DVI ADPCM --------------------------------------------------------------------------------------------------------------------------
KLATT_RES_HD int codec_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// The decoder's step, which the encoder shares: code (0 .. 15) at the step of idx moves val and idx
KLATT_RES_HD void adpcm_apply(int code, int step, int& val, int& idx)
{
    int vp = step >> 3;
    if (code & 4) vp += step;
    if (code & 2) vp += step >> 1;
    if (code & 1) vp += step >> 2;
    val = codec_clamp((code & 8) ? val - vp : val + vp, -32768, 32767);
    const int delta = code & 7;
    idx = codec_clamp(idx + (delta < 4 ? -1 : 2 * (delta - 3)), 0, kAdpcmSteps - 1);      // INDEX = -1 -1 -1 -1 2 4 6 8
}
// One sample s at the step of idx: its code; val (the decoded sample) and idx move on
KLATT_RES_HD int adpcm_encode(int s, int step, int& val, int& idx)
{
    int diff = s - val;
    const int sign = diff < 0 ? 8 : 0;
    if (sign) diff = -diff;
    int delta = 0;
    if (diff >= step) { delta = 4; diff -= step; }
    if (diff >= (step >> 1)) { delta |= 2; diff -= step >> 1; }
    if (diff >= (step >> 2)) delta |= 1;
    const int code = delta | sign;
    adpcm_apply(code, step, val, idx);
    return code;
}

// ---- the host's statements: the shared functions in plain loops ------------------------------------------------------------------------------
inline void codec_put(void* decoded, int format, long long n, int d)
{
    if (!decoded) return;
    if (format) static_cast<float*>(decoded)[n] = codec_value<true>(d); else static_cast<int16_t*>(decoded)[n] = codec_value<false>(d);
}

// decoded: float[length] (format 1) or int16_t[length] (format 0), codes: uint8_t[length]; either may be null.  state (may be null): the
// ADPCM encoder's val and idx behind the last sample (0 0 for a G.711 law).
template <typename In>
inline void code_host(const In* x, long long length, int codec, int format, void* decoded, uint8_t* codes, int* state)
{
    int val = 0, idx = 0;
    for (long long n = 0; n < length; ++n) {
        const int s = codec_sample(x[n]);
        int code, d;
        if (codec == kCodecUlaw) { code = ulaw_encode(s); d = ulaw_decode(code); }
        else if (codec == kCodecAlaw) { code = alaw_encode(s); d = alaw_decode(code); }
        else { code = adpcm_encode(s, kAdpcmTable.step[idx], val, idx); d = val; }
        if (codes) codes[n] = (uint8_t)code;
        codec_put(decoded, format, n, d);
    }
    if (state) { state[0] = val; state[1] = idx; }
}

// The decoder alone.  The first ADPCM code above 15, or -1
inline long long decode_bad_code(const uint8_t* codes, long long length, int codec)
{
    for (long long n = 0; codec == kCodecAdpcm && n < length; ++n) if (codes[n] > 15) return n;
    return -1;
}
inline void decode_host(const uint8_t* codes, long long length, int codec, int format, void* out, int* state)
{
    int val = 0, idx = 0;
    for (long long n = 0; n < length; ++n) {
        int d;
        if (codec == kCodecUlaw) d = ulaw_decode(codes[n]);
        else if (codec == kCodecAlaw) d = alaw_decode(codes[n]);
        else { adpcm_apply(codes[n], kAdpcmTable.step[idx], val, idx); d = val; }
        codec_put(out, format, n, d);
    }
    if (state) { state[0] = val; state[1] = idx; }
}

// What klatt_code_adpcm puts out: bit 0 the decoded samples, bit 1 the codes
constexpr int kCodeDecoded = 1, kCodeCodes = 2;
// Dwords between the rows of its LDS region, and the dword of a row its codes are staged from
constexpr int codec_pitch(int outputs) { return outputs == (kCodeDecoded | kCodeCodes) ? kCodecPitchBoth : kFilterPitch; }
constexpr int codec_codes_at(int outputs) { return outputs == (kCodeDecoded | kCodeCodes) ? kFilterTile : 0; }
// Lanes a row's staged run of kFilterTile elements takes in codec_store_rows: the aligned 16 bytes it can touch, rounded up to a power of two
template <typename T> constexpr int kCodecStoreLanes = sizeof(T) == 4 ? 32 : sizeof(T) == 2 ? 16 : 8;

// Lane `lane` of the wavefront's stores of the tile at t0, as far as row q is concerned: its values staged at `staged`, its first element
// in the output `dst`, its outputs `outLen`.  Lane i of the row's kCodecStoreLanes takes the i-th aligned 16 bytes (tile_store_lane).
template <typename T>
KLATT_RES_HD void codec_store_row(T* out, int mis, long long dst, long long outLen, long long rowStride, long long t0, const T* staged, int i)
{
    static_assert(kFilterTile / kTileLane<T> + 1 <= kCodecStoreLanes<T>, "a row's run fits its lanes");
    const int n = tile_n(rowStride, outLen, t0, kFilterTile);
    if (n <= 0 || i >= tile_lanes<T>(mis, dst + t0, n)) return;
    tile_store_lane(out, mis, dst + t0, n, staged, i);
}

// ---- the G.711 kernel's writer: the run staged where its 16-byte blocks are the output's --------------------------------------------------
// The elements e0 .. e0 + count - 1 are staged from index codec_lead, what e0 lies past the aligned 16 bytes that hold it, so that staged
// block i (elements i EL .. i EL + EL - 1 of `staged`, itself 16-byte aligned) is the i-th aligned 16 bytes of the output the run touches:
// one 16-byte LDS read and, where the run covers the block, one 16-byte store; the run's two ends go element by element.
// The sample a lane of a tile that begins inside a row of len samples loads for sample s >= 0: s itself, or the row's last
KLATT_RES_HD long long codec_within(long long s, long long len) { return s < len ? s : len - 1; }
template <typename T> KLATT_RES_HD int codec_lead(int mis, long long e0) { return (int)(e0 - tile_first<T>(mis, e0)); }
template <typename T> KLATT_RES_HD int codec_blocks(int lead, int count) { return (lead + count + kTileLane<T> - 1) / kTileLane<T>; }
template <typename T> KLATT_RES_HD void codec_store_block(T* out, long long e0, int lead, int count, const T* staged, int i)
{
    constexpr int EL = kTileLane<T>;
    struct alignas(16) Lane { T x[EL]; };
    const int j0 = i * EL;                                   // the block's first staged index; its first element is e0 - lead + j0
    const Lane l = *reinterpret_cast<const Lane*>(staged + j0);
    T* o = out + (e0 - lead + j0);
    if (j0 >= lead && j0 + EL <= lead + count) *reinterpret_cast<Lane*>(o) = l;
    else {
        for (int q = 0; q < EL; ++q) if (j0 + q >= lead && j0 + q < lead + count) o[q] = l.x[q];
    }
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct CodeArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const ResRow* rows;                  // (outLen is len)
    TileOut tile;                        // tile.out: the decoded samples, or null
    uint8_t* codes;                      // or null
};

template <int LAW, bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_code_g711(const CodeArgs A)
{
    using T = TileValue<F32>;
    constexpr int PER = kCodeTile / 256;      // samples of a tile a lane takes: i = tid, tid + 256, ...
    __shared__ __attribute__((aligned(16))) T staged[kCodeTile + kTileLane<T>];
    __shared__ __attribute__((aligned(16))) uint8_t stagedCodes[kCodeTile + kTileLane<uint8_t>];
    const int tid = threadIdx.x;
    T* const decoded = static_cast<T*>(A.tile.out);
    const int misD = tile_mis<T>(decoded), misC = tile_mis<uint8_t>(A.codes);
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, kCodeTile, r, t0);
        const ResRow row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.outLen, t0, kCodeTile);
        const long long e0 = row.dst + t0;
        const int leadD = decoded ? codec_lead<T>(misD, e0) : 0, leadC = A.codes ? codec_lead<uint8_t>(misC, e0) : 0;
        if (t0 < row.len) {
            const In* __restrict__ x = static_cast<const In*>(A.in) + row.src;
            In v[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {      // the lane's loads together and without a branch: past the row's end its last sample again, unused
                const long long s = t0 + tid + 256 * k;
                v[k] = x[codec_within(s, row.len)];
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = tid + 256 * k;
                if (i >= n) break;
                const bool inside = tile_inside(t0 + i, row.len);
                const int code = g711_encode<LAW>(codec_sample(v[k]));
                staged[leadD + i] = inside ? codec_value<F32>(g711_decode<LAW>(code)) : (T)0;      // (past the row: +0 and code 0, the padding)
                stagedCodes[leadC + i] = inside ? (uint8_t)code : (uint8_t)0;
            }
        } else {                                  // (a padded row's tile past its end: +0 and code 0 without loads or arithmetic)
            for (int i = tid; i < n; i += 256) { staged[leadD + i] = (T)0; stagedCodes[leadC + i] = (uint8_t)0; }
        }
        __syncthreads();
        if (decoded) for (int i = tid; i < codec_blocks<T>(leadD, n); i += 256) codec_store_block(decoded, e0, leadD, n, staged, i);
        if (A.codes) for (int i = tid; i < codec_blocks<uint8_t>(leadC, n); i += 256) codec_store_block(A.codes, e0, leadC, n, stagedCodes, i);
        __syncthreads();      // every lane has read the staged values before the next tile's
    }
}

struct AdpcmArgs {
    const void* in;                      // as CodeArgs'
    const FilterRow* rows;               // the packed table (klatt_filter.h: a section each, fillers none)
    const FilterGroup* groups;
    long long nGroups;
    long long rowStride;                 // the padded form: a row's width
    void* decoded;                       // or null, as OUT says
    uint8_t* codes;
};

// The wavefront's stores of the tile at t0: row q of the group has its values staged at region + q PITCH + AT dwords, its first element in
// the output (-1: a filler) and its outputs in where[q]
template <typename T, int PITCH, int AT>
__device__ __forceinline__ void codec_store_rows(void* out, const long long (*where)[2], long long rowStride, long long t0, const int* region, int lane)
{
    constexpr int PER = kCodecStoreLanes<T>;
    const int mis = tile_mis<T>(out), sub = lane / PER, i = lane % PER;
    for (int q0 = 0; q0 < kFilterLanes; q0 += kFilterLanes / PER) {
        const int q = q0 + sub;
        const long long dst = where[q][0];
        if (dst < 0) continue;
        codec_store_row(static_cast<T*>(out), mis, dst, where[q][1], rowStride, t0, reinterpret_cast<const T*>(region + q * PITCH + AT), i);
    }
}

template <int OUT, bool F32, typename In = int16_t>
__global__ void __launch_bounds__(kFilterLanes) klatt_code_adpcm(const AdpcmArgs A)
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
        const FilterRow me = A.rows[G.first + lane];
        int val = 0, idx = 0;
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
                // the next tile's loads, in flight during the steps (none where no row of the group reaches it)
                if (t0 + TILE < G.inMost) filter_load_rows(next, in, me.src, me.len, t0 + TILE, lane);
                else {
#pragma unroll
                    for (int q = 0; q < kFilterLanes; ++q) next[q] = (In)0;
                }
                __syncthreads();
                const long long live = me.outLen - t0;             // samples of the tile inside the lane's row; the rest is padding
                for (int t = 0; t < TILE; ++t) {
                    const int code = adpcm_encode(mine[t], steps[idx], val, idx);
                    if (DECODED) staged[t] = t < live ? codec_value<F32>(val) : (T)0;
                    if (CODES) stagedCodes[t] = t < live ? (uint8_t)code : (uint8_t)0;
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
        __syncthreads();                                           // the last tile has left before the next group's first
    }
}

}  // namespace klatt
#endif
