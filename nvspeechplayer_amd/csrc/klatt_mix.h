// klatt_mix.h -- a batch's PCM mixed with noise clips and other utterances at set levels (speechPlayer_batch_exportMixed), the exact power
// of utterances (speechPlayer_batch_exportPower), the batch's noise bank (speechPlayer_batch_setNoiseBank) and the same mixture of plain PCM
// on the host (speechPlayer_pcmMix); the same onto the rows of a caller's signal (speechPlayer_batch_exportMixedOf, exportPowerOf,
// speechPlayer_signalMix, speechPlayer_signalPower), whose power is klatt_sigpower.h's.
//
// The definition.  For a row whose utterance has L samples of int16 PCM s(t):
//   input      x[n] = res_input(s(n)) (klatt_resample.h: the bits of speechPlayer_batch_exportPcm's format 1).  The output has L samples, on
//              the grid of the other exports; there is no tail.
//   sources    a CLIP of the batch's noise bank: float32 c[0 .. N-1], 1 <= N < 2^31, every value finite and at most 2^16 in magnitude; or
//              an UTTERANCE of the same batch: x_u[n] = res_input(s_u(n)), N = L_u -- it may be the row's own.
//   powers     of an utterance: S_u = sum s_u(n)^2, an exact unsigned 64-bit integer (order-free: any reduction gives the same bits), and
//              P_u = mix_power(S_u, L_u) = (double)S_u / (double)L_u / 1073676289.0 (32767^2), 0 for L_u = 0.  Of a clip:
//              P_c = (sum over n ascending of (double)c[n] * (double)c[n]) / N, computed once on the host when the bank is set and kept
//              with it.  Both are WHOLE-SIGNAL mean squares, silences included: an utterance that is half pauses is 3 dB "quieter" than
//              its speech.
//   placement  of term j, mix_source_index: loop = 1: v_j[m] = src[(offset + m) mod N], 0 <= offset < N.  loop = 0: v_j[m] = src[m - offset]
//              where 0 <= m - offset < N, else +0, |offset| <= 2^44; a negative offset skips the source's beginning.
//   level      of term j: levelKind 1: g_j = (float)level, finite, |level| <= 2^32.  levelKind 0: level is an SNR in dB, finite,
//              |level| <= 200; ratio = pow(10.0, level / 10.0) is evaluated on the HOST for both statements (as the spectrogram's twiddles
//              are) and g_j = mix_gain(Ps, Pv, ratio) = (Ps > 0 && Pv * ratio > 0) ? (float)fmin(sqrt(Ps / (Pv * ratio)), 2^32) : 0.0f:
//              one binary64 product, one quotient and one square root, each IEEE on both sides, then one rounding to binary32.  Ps is the
//              power of the row's own utterance at gain 1, whatever speechGain is.
//   output     acc = speechGain * x[m] (one binary32 product; speechGain finite, at most 2^32 in magnitude); for j ascending
//              acc = conv_step(acc, v_j[m], g_j) (klatt_convolve.h: one fmaf); y[m] = conv_finish(acc).  Format 1 is y[m], format 0
//              res_int16(y[m]).  With at most kMixMaxTerms = 64 terms per row no sum overflows under the bounds above, and the
//              convolution's lemma holds: a term whose product is +-0 may be dropped without changing a bit, so a kernel may skip a term
//              that lies wholly outside a tile.
// The result is a function of the batch's PCM: it needs a synthesis launch, depends on the mode and is ordered as speechPlayer_batch_exportPcm
// is.
// Onto a signal (speechPlayer_batch_exportMixedOf): "the utterance's int16 PCM" becomes "the row's samples", int16 or float32 (tile_x is
// the conversion); a kind-1 term names a ROW OF THE SAME SIGNAL, chosen or not, the row's own included; the power of a row is
// signal_power (klatt_sigpower.h: the pool's exact integer sum for int16 rows, the fixed tree for float32 ones), and everything after the
// powers -- mix_gain, the placement, the fmaf chain -- is unchanged.  The speech stands behind a room, the noise is added at an SNR
// against the reverberant speech.  With an int16 signal that is the pool, every bit is the pool export's.
// Out of scope: a term from a different signal or from the pool in a mix onto a signal; live handles; NodePlayer, which reaches the
// export through speechPlayer_node_part; segment or active-speech (VAD-weighted) levels; loudness weighting; random draws of any kind --
// clips, offsets and levels are the caller's.
//
//   The plan        mix_bank_plan (the bank, its refusals, the clip powers), mix_check_term / mix_check_row (the refusals of a term and of
//                   a row's place in termStart; messages without the entry point's prefix).
//   The statement   mix_host: the definition in a plain loop over the shared functions.
//   The indices     What the kernel visits, as plain functions a stand-alone program checks against brute force (tests/native/check_mix.cpp):
//                   mix_term_first, mix_term_last, mix_term_skipped, mix_loop_start, mix_loop_index, mix_lane_start, mix_lane_whole,
//                   mix_speech_whole; the tiles themselves are klatt_tiles.h's.
//   klatt_power     S_u of the distinct utterances a call needs into zeroed uint64 slots: a workgroup takes kPowerTile samples of one
//                   utterance, lanes take 16-byte loads of eight samples where the address allows, accumulate in 64 bits (a square is up
//                   to 2^30: two of them do not fit a signed 32-bit sum), the wavefront reduces, one 64-bit atomic add per wavefront.
//   klatt_mix_gains one lane per term: mix_gain from the slots and the bank's powers, into the call's scratch and the caller's deviceGains.
//                   klatt_mix_gains_of is the same from an array of binary64 powers per slot, which a signal's rows have:
//                   klatt_signal_power and its row pass make it for float32 rows, klatt_power and klatt_power_doubles for int16 ones.
//   klatt_mix       A 256-lane workgroup takes tiles of kMixTile consecutive outputs of one row (klatt_tiles.h: the walk); lane l owns
//                   the FOUR outputs 4 l .. 4 l + 3.  The row's term descriptors are wave-uniform.  Per term and tile the start index
//                   (offset + t0) mod N is computed once; the lanes wrap by comparison when N >= kMixTile and by a 32-bit remainder
//                   below that.  A term wholly outside the tile is skipped.  The values go out as klatt_tiles.h says (the writer):
//                   staged in LDS in the output's type, a padded row's remainder as +0.  The kernel is a template on the element of the
//                   speech row and of the kind-1 terms, int16 (the pool; an int16 signal) or float32; four consecutive elements go in
//                   one load where they are aligned and whole.
#pragma once

#include "klatt_convolve.h"
#include "klatt_sigpower.h"

namespace klatt {

constexpr int kMixTile = 1024;                          // consecutive outputs of one row a workgroup takes at a time (4 per lane)
constexpr int kMixMaxTerms = 64;                        // of one row
constexpr long long kMixMaxCallTerms = 1ll << 22;       // of one call
constexpr long long kMixMaxClips = 1ll << 20;           // of a bank
constexpr long long kMixMaxBank = 1ll << 28;            // samples of a bank (1 GB)
constexpr long long kMixMaxOffset = 1ll << 44;          // |offset| of a term that does not loop
constexpr long long kMixMaxLength = 1ll << 33;          // samples of plain PCM the host statement takes: S_u stays below 2^64
constexpr float kMixMaxClipValue = 65536.0f;            // |c[n]| <= 2^16
constexpr double kMixMaxGain = 4294967296.0;            // |g_j| <= 2^32, |speechGain| <= 2^32
constexpr double kMixMaxDb = 200.0;                     // |SNR|
constexpr double kMixFullScale2 = 1073676289.0;         // 32767^2: the power of a full-scale square wave of x is 1
constexpr int kPowerTile = 8192;                        // samples of one utterance a workgroup of klatt_power sums at a time

static_assert(kMixTile == 4 * 256 && kPowerTile % (8 * 256) == 0, "four outputs per lane; whole 16-byte loads per lane");

// The layout of speechPlayer_mixTerm_t (include/speechPlayer_batch.h), which this header does not include
struct MixTermIn { int kind, levelKind; long long source, offset; double level; int loop, reserved; };
static_assert(sizeof(MixTermIn) == 40, "speechPlayer_mixTerm_t");

// ---- the definition's functions, host and device from one source ---------------------------------------------------------------------------
KLATT_RES_HD double mix_power(unsigned long long S, long long L) { return L > 0 ? (double)S / (double)L / kMixFullScale2 : 0.0; }

KLATT_RES_HD float mix_gain(double Ps, double Pv, double ratio)
{
    const double d = Pv * ratio;
    if (!(Ps > 0.0 && d > 0.0)) return 0.0f;
    const double g = sqrt(Ps / d);
    return (float)(g < kMixMaxGain ? g : kMixMaxGain);      // fmin(g, 2^32): g is no NaN here
}

// The element of a source of N samples that output m of term (offset, loop) reads, or -1: it reads +0
KLATT_RES_HD long long mix_source_index(long long m, long long offset, long long N, int loop)
{
    if (loop) return (offset + m) % N;
    const long long i = m - offset;
    return i >= 0 && i < N ? i : -1;
}

// ---- the kernel's index arithmetic ---------------------------------------------------------------------------------------------------------
// A term that does not loop covers the outputs [first, last) of the tile at t0 with `live` outputs inside the row, in the tile's own
// numbering (first >= last: none); output o reads element t0 - offset + o
KLATT_RES_HD int mix_term_first(long long t0, long long offset) { return offset > t0 ? (int)(offset - t0 < kMixTile ? offset - t0 : kMixTile) : 0; }
KLATT_RES_HD int mix_term_last(long long t0, int live, long long offset, long long N)
{
    const long long end = offset + N - t0;      // (|offset| <= 2^44, N < 2^44, t0 < 2^50)
    return end < live ? (int)(end > 0 ? end : 0) : live;
}
KLATT_RES_HD bool mix_term_skipped(long long t0, int live, long long offset, long long N, int loop)
{
    return live <= 0 || (!loop && mix_term_first(t0, offset) >= mix_term_last(t0, live, offset, N));
}
// A looped term: output o of the tile reads element mix_loop_index(mix_loop_start(offset, t0, N), o, N)
KLATT_RES_HD long long mix_loop_start(long long offset, long long t0, long long N) { return (offset + t0) % N; }
KLATT_RES_HD long long mix_loop_index(long long k0, int o, long long N)
{
    if (N >= kMixTile) { const long long i = k0 + o; return i >= N ? i - N : i; }      // (k0 < N, o < kMixTile <= N: one wrap at most)
    return (long long)((uint32_t)(k0 + o) % (uint32_t)N);
}
// The element a lane's first output o0 = 4 l reads, where `base` is mix_loop_start (looped) or t0 - offset: wrapped once for N >= kMixTile
KLATT_RES_HD long long mix_lane_start(long long base, int o0, long long N, int loop)
{
    const long long i0 = base + o0;
    return loop && N >= kMixTile && i0 >= N ? i0 - N : i0;
}
// The lane's four outputs o0 .. o0 + 3 lie inside the term's cover [lo, hi) and read the four CONSECUTIVE elements i0 .. i0 + 3 of the
// source: one load takes them.  Never for a looped source shorter than a tile (its lanes wrap by remainder, element by element).
KLATT_RES_HD bool mix_lane_whole(int o0, int lo, int hi, long long i0, long long N, int loop)
{
    return !(loop && N < kMixTile) && o0 >= lo && o0 + 4 <= hi && i0 >= 0 && i0 + 4 <= N;
}

// The lane's four samples of speech at p = the tile's first sample + o0 are all inside the row and p is aligned to the four (8 bytes of
// int16, 16 of float32): one load takes them (an utterance starts on 64 bytes of the pool and a tile on 2048 of the utterance, so there
// this fails only at a row's ragged end; a signal's row starts wherever its table says)
template <typename In> KLATT_RES_HD bool mix_speech_whole(const In* p, int o0, int live) { return o0 + 4 <= live && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(In) - 1)) == 0; }

// ---- the bank ------------------------------------------------------------------------------------------------------------------------------
struct MixBank {
    std::vector<long long> start;      // [nClips + 1]
    std::vector<double> power;         // [nClips] P_c
    long long clips() const { return (long long)power.size(); }
};

inline double mix_clip_power(const float* c, long long N)
{
    double acc = 0.0;
    for (long long n = 0; n < N; ++n) acc += (double)c[n] * (double)c[n];
    return acc / (double)N;
}

// The first value of c[0 .. N) that is not finite or above 2^16 in magnitude, or -1
inline long long mix_bad_value(const float* c, long long N)
{
    for (long long n = 0; n < N; ++n)
        if (!(fabsf(c[n]) <= kMixMaxClipValue)) return n;      // (a NaN fails the comparison)
    return -1;
}

// The bank of a request (nNoise = 0: none), or false with `why` set
inline bool mix_bank_plan(MixBank& B, const float* noise, const long long* noiseStart, long long nNoise, std::string& why)
{
    char buf[200];
    B.start.clear(); B.power.clear();
    if (nNoise < 0 || nNoise > kMixMaxClips) { snprintf(buf, sizeof buf, "%lld clips (0 .. 2^20)", nNoise); why = buf; return false; }
    if (nNoise == 0) return true;
    if (!noise || !noiseStart) { why = "no clips (noise and noiseStart)"; return false; }
    if (noiseStart[0] != 0) { snprintf(buf, sizeof buf, "noiseStart[0] = %lld (the first clip starts at 0)", noiseStart[0]); why = buf; return false; }
    for (long long k = 0; k < nNoise; ++k) {
        const long long a = noiseStart[k], b = noiseStart[k + 1];
        if (b <= a) { snprintf(buf, sizeof buf, "noiseStart[%lld] = %lld is not above noiseStart[%lld] = %lld (a clip has at least 1 sample)", k + 1, b, k, a); why = buf; return false; }
        if (b > kMixMaxBank) { snprintf(buf, sizeof buf, "the clips have more than %lld samples in all", kMixMaxBank); why = buf; return false; }
    }
    for (long long k = 0; k < nNoise; ++k) {
        const long long bad = mix_bad_value(noise + noiseStart[k], noiseStart[k + 1] - noiseStart[k]);
        if (bad >= 0) {
            snprintf(buf, sizeof buf, "sample %lld of clip %lld is %g (finite, at most 2^16 in magnitude)", bad, k, (double)noise[noiseStart[k] + bad]);
            why = buf; return false;
        }
    }
    B.start.assign(noiseStart, noiseStart + nNoise + 1);
    B.power.resize((size_t)nNoise);
    for (long long k = 0; k < nNoise; ++k) B.power[(size_t)k] = mix_clip_power(noise + noiseStart[k], noiseStart[k + 1] - noiseStart[k]);
    return true;
}

// ---- the refusals of a request ----------------------------------------------------------------------------------------------------------------
// Row i's place in termStart: its first term and its count, or false with `why` set
inline bool mix_check_row(const long long* termStart, long long i, const void* terms, std::string& why)
{
    char buf[200];
    if (!termStart) { why = "no termStart"; return false; }
    if (i == 0 && termStart[0] != 0) { snprintf(buf, sizeof buf, "termStart[0] = %lld (the first row's terms start at 0)", termStart[0]); why = buf; return false; }
    const long long a = termStart[i], b = termStart[i + 1];
    if (b < a) { snprintf(buf, sizeof buf, "termStart[%lld] = %lld is below termStart[%lld] = %lld", i + 1, b, i, a); why = buf; return false; }
    if (b - a > kMixMaxTerms) { snprintf(buf, sizeof buf, "row %lld has %lld terms (at most %d)", i, b - a, kMixMaxTerms); why = buf; return false; }
    if (b > kMixMaxCallTerms) { snprintf(buf, sizeof buf, "more than %lld terms in all (row %lld)", kMixMaxCallTerms, i); why = buf; return false; }
    if (b > a && !terms) { snprintf(buf, sizeof buf, "row %lld has %lld terms and there are none (terms)", i, b - a); why = buf; return false; }
    return true;
}

// A term of row i against its source: nClips (-1: no bank is set) and nUtterances are what `source` may name, N the source's length where
// it names one (the caller looks it up once this has passed the range checks: lengthOf(kind, source)).  False with `why` set: the
// message names row and term.  ofSignal: a kind-1 source is a row of the signal the mix is made onto.
template <class LengthOf>
bool mix_check_term(const MixTermIn& t, long long i, long long j, long long nClips, long long nUtterances, LengthOf lengthOf, std::string& why, bool ofSignal = false)
{
    char buf[256], at[64];
    at[0] = 0;
    const auto where = [&]() -> const char* { snprintf(at, sizeof at, "row %lld, term %lld", i, j); return at; };      // (only a refusal pays for it)
    if (t.kind != 0 && t.kind != 1) { snprintf(buf, sizeof buf, "%s: kind %d (0 a bank clip, 1 an utterance of the batch)", where(), t.kind); why = buf; return false; }
    if (t.levelKind != 0 && t.levelKind != 1) { snprintf(buf, sizeof buf, "%s: levelKind %d (0 an SNR in dB, 1 a linear gain)", where(), t.levelKind); why = buf; return false; }
    if (t.loop != 0 && t.loop != 1) { snprintf(buf, sizeof buf, "%s: loop %d (0 or 1)", where(), t.loop); why = buf; return false; }
    if (t.kind == 0) {
        if (nClips < 0) { snprintf(buf, sizeof buf, "%s: clip %lld, and no noise bank is set", where(), t.source); why = buf; return false; }
        if (t.source < 0 || t.source >= nClips) { snprintf(buf, sizeof buf, "%s: clip %lld is not in the bank (%lld clips)", where(), t.source, nClips); why = buf; return false; }
    } else if (t.source < 0 || t.source >= nUtterances) {
        snprintf(buf, sizeof buf, "%s: source %lld is not %s (%lld)", where(), t.source, ofSignal ? "a row of the signal" : "an utterance of the batch", nUtterances); why = buf; return false;
    }
    const long long N = lengthOf(t.kind, t.source);
    if (t.loop) {
        if (N == 0) { snprintf(buf, sizeof buf, "%s: a looped source of length 0", where()); why = buf; return false; }
        if (t.offset < 0 || t.offset >= N) { snprintf(buf, sizeof buf, "%s: offset %lld of a looped source of %lld samples (0 .. N-1)", where(), t.offset, N); why = buf; return false; }
    } else if (t.offset < -kMixMaxOffset || t.offset > kMixMaxOffset) {
        snprintf(buf, sizeof buf, "%s: offset %lld (at most 2^44 in magnitude)", where(), t.offset); why = buf; return false;
    }
    if (t.levelKind == 1 && !(fabs(t.level) <= kMixMaxGain)) { snprintf(buf, sizeof buf, "%s: gain %g (finite, at most 2^32 in magnitude)", where(), t.level); why = buf; return false; }
    if (t.levelKind == 0 && !(fabs(t.level) <= kMixMaxDb)) { snprintf(buf, sizeof buf, "%s: an SNR of %g dB (finite, at most 200 in magnitude)", where(), t.level); why = buf; return false; }
    return true;
}

inline bool mix_check_speech_gain(float g, long long i, std::string& why)
{
    if (fabs((double)g) <= kMixMaxGain) return true;
    char buf[128];
    snprintf(buf, sizeof buf, "row %lld: speechGain %g (finite, at most 2^32 in magnitude)", i, (double)g);
    why = buf;
    return false;
}

// The ratio of an SNR term, evaluated on the host for both statements
inline double mix_ratio(double db) { return pow(10.0, db / 10.0); }

// ---- the host's statement (speechPlayer_pcmMix): the shared functions in a plain loop --------------------------------------------------------
struct MixSource { const void* data; long long length; int isFloat; double power; };      // int16 PCM (an utterance) or float32 (a clip; a signal's row)
struct MixTermHost { int source; long long offset; int loop; float gain; };

inline unsigned long long mix_square_sum(const int16_t* s, long long L)
{
    unsigned long long S = 0;
    for (long long n = 0; n < L; ++n) S += (unsigned long long)((long long)s[n] * (long long)s[n]);
    return S;
}

// The power of a signal's row (klatt_sigpower.h: the definition): format 0 int16, 1 float32
inline double signal_power(const void* x, int format, long long L)
{
    return format ? sig_power_host(static_cast<const float*>(x), L) : mix_power(mix_square_sum(static_cast<const int16_t*>(x), L), L);
}

KLATT_RES_HD float mix_source_value(const void* data, int isFloat, long long i)
{
    return isFloat ? static_cast<const float*>(data)[i] : res_input((int)static_cast<const int16_t*>(data)[i]);
}

// format 1: out is float[length]; format 0: int16_t[length].  Returns length.
template <typename In>
inline long long mix_host(const In* pcm, long long length, float speechGain, const MixSource* sources, const MixTermHost* terms, long long nTerms,
                          int format, void* out)
{
    for (long long m = 0; m < length; ++m) {
        float acc = speechGain * tile_x(pcm[m]);
        for (long long j = 0; j < nTerms; ++j) {
            const MixSource& s = sources[terms[j].source];
            const long long i = mix_source_index(m, terms[j].offset, s.length, terms[j].loop);
            acc = conv_step(acc, i >= 0 ? mix_source_value(s.data, s.isFloat, i) : 0.0f, terms[j].gain);
        }
        res_store(out, format, m, conv_finish(acc));
    }
    return length;
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

// ---- klatt_power ----
struct PowerArgs {
    const int16_t* pool;
    const PowerJob* jobs;
    const long long* tileStart;      // [nJobs + 1] the first tile of every job
    long long nJobs, nTiles;
    unsigned long long* slots;       // [nJobs], zero before the launch
};

__device__ __forceinline__ unsigned long long power_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ void __launch_bounds__(256) klatt_power(const PowerArgs A)
{
    const int tid = threadIdx.x;
    for (long long g = blockIdx.x; g < A.nTiles; g += gridDim.x) {
        long long r, j;
        packed_locate(g, A.tileStart, A.nJobs, r, j);      // (a job of no samples has no tiles: the last job that starts here is the one)
        const PowerJob job = A.jobs[r];
        const long long s0 = j * kPowerTile;
        const int n = (int)min((long long)kPowerTile, job.len - s0);
        const int16_t* __restrict__ p = A.pool + job.src + s0;
        unsigned long long acc = 0;
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const int n8 = n >> 3;
            const int4* __restrict__ p8 = reinterpret_cast<const int4*>(p);
            for (int i = tid; i < n8; i += 256) {
                const int4 w = p8[i];
                const int e[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int a = (int)(int16_t)(e[q] & 0xFFFF), c = e[q] >> 16;
                    acc += (unsigned long long)(unsigned)(a * a) + (unsigned long long)(unsigned)(c * c);
                }
            }
            done = n8 << 3;
        }
        for (int i = done + tid; i < n; i += 256) { const int a = p[i]; acc += (unsigned long long)(unsigned)(a * a); }
        acc = power_wave_sum(acc);
        if ((tid & 63) == 0 && acc) atomicAdd(A.slots + r, acc);
    }
}

// exportPower's deal-out: row i takes the sum of its utterance's slot
__global__ void __launch_bounds__(256) klatt_power_deal(const unsigned long long* __restrict__ slots, const long long* __restrict__ slotOf, long long n,
                                                        unsigned long long* __restrict__ out)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) out[i] = slots[slotOf[i]];
}

// int16 signals: the exact sums of klatt_power as the binary64 powers everything downstream of a signal's powers reads
__global__ void __launch_bounds__(256) klatt_power_doubles(const unsigned long long* __restrict__ slots, const PowerJob* __restrict__ jobs, long long n,
                                                           double* __restrict__ powers)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) powers[i] = mix_power(slots[i], jobs[i].len);
}

// ---- klatt_mix_gains ----
// A term's level: linear (gain as given) or an SNR (ratio; the row's slot; the source's slot, or -1: a clip of power pv)
struct MixGainJob { double ratio, pv; long long rowSlot, srcSlot; float gain; int linear; };

__global__ void __launch_bounds__(256) klatt_mix_gains(const MixGainJob* __restrict__ jobs, long long nTerms, const unsigned long long* __restrict__ slots,
                                                       const PowerJob* __restrict__ slotJobs, float* __restrict__ gains, float* __restrict__ deviceGains)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nTerms; i += gridDim.x * 256ll) {
        const MixGainJob job = jobs[i];
        float g = job.gain;
        if (!job.linear) {
            const double Ps = mix_power(slots[job.rowSlot], slotJobs[job.rowSlot].len);
            const double Pv = job.srcSlot >= 0 ? mix_power(slots[job.srcSlot], slotJobs[job.srcSlot].len) : job.pv;
            g = mix_gain(Ps, Pv, job.ratio);
        }
        gains[i] = g;
        if (deviceGains) deviceGains[i] = g;
    }
}

// The same over a signal's rows: Ps and Pv from the call's binary64 powers, one per slot, or the bank's P_c
__global__ void __launch_bounds__(256) klatt_mix_gains_of(const MixGainJob* __restrict__ jobs, long long nTerms, const double* __restrict__ powers,
                                                          float* __restrict__ gains, float* __restrict__ deviceGains)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nTerms; i += gridDim.x * 256ll) {
        const MixGainJob job = jobs[i];
        float g = job.gain;
        if (!job.linear) g = mix_gain(powers[job.rowSlot], job.srcSlot >= 0 ? powers[job.srcSlot] : job.pv, job.ratio);
        gains[i] = g;
        if (deviceGains) deviceGains[i] = g;
    }
}

// ---- klatt_mix ----
constexpr int kMixClip = 1, kMixLoop = 2;      // MixTermDev.flags
// A term as the kernel reads it: the source's first element (in the bank: kMixClip; else in the pool or the signal), its samples, the offset
struct MixTermDev { long long at, len, offset; int flags, pad; };
// first element (of the pool, of the signal's data) and samples of a row; its first element in the output; its first term, its terms; its speech gain
struct MixRow { long long src, len, dst, term0; int nTerms; float speechGain; };

struct MixArgs {
    const void* pool;                // the pool, or a signal's data: elements of the kernel's In
    const float* bank;
    const MixRow* rows;
    TileOut tile;
    const MixTermDev* terms;
    const float* gains;
};

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_mix(const MixArgs A)
{
    using T = TileValue<F32>;
    constexpr int TILE = kMixTile;
    __shared__ __attribute__((aligned(16))) T staged[TILE];
    struct __attribute__((packed, aligned(4))) F4 { float x[4]; };      // four floats at any float's address
    struct __attribute__((packed, aligned(2))) S4 { int16_t x[4]; };    // four samples at any sample's address
    using I4 = typename std::conditional<std::is_same<In, float>::value, F4, S4>::type;
    const In* __restrict__ const pool = static_cast<const In*>(A.pool);
    const int tid = threadIdx.x;
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, TILE, r, t0);
        const MixRow row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.len, t0, TILE);
        const int live = tile_live(n, row.len, t0);      // outputs of the tile inside the row; the rest is padding
        const int o0 = 4 * tid;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live > 0) {
            // ---- the speech: acc = speechGain * x ----
            const In* __restrict__ pcm = pool + row.src + t0;
            if (mix_speech_whole(pcm + o0, o0, live)) {
                struct alignas(4 * sizeof(In)) S4A { In x[4]; };
                const S4A s = *reinterpret_cast<const S4A*>(pcm + o0);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = row.speechGain * tile_x(s.x[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (o0 + q < live) acc[q] = row.speechGain * tile_x(pcm[o0 + q]);
            }
            // ---- the terms, ascending (every condition on the term is uniform over the workgroup) ----
            for (int jt = 0; jt < row.nTerms; ++jt) {
                const MixTermDev t = A.terms[row.term0 + jt];
                const float gain = A.gains[row.term0 + jt];
                const int loop = (t.flags & kMixLoop) ? 1 : 0;
                if (mix_term_skipped(t0, live, t.offset, t.len, loop)) continue;
                const int lo = loop ? 0 : mix_term_first(t0, t.offset), hi = loop ? live : mix_term_last(t0, live, t.offset, t.len);
                const long long base = loop ? mix_loop_start(t.offset, t0, t.len) : t0 - t.offset;      // output o reads element base + o, wrapped
                const long long i0 = mix_lane_start(base, o0, t.len, loop);
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (mix_lane_whole(o0, lo, hi, i0, t.len, loop)) {      // four consecutive elements inside the source
                    if (t.flags & kMixClip) {
                        const F4 c = *reinterpret_cast<const F4*>(A.bank + t.at + i0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = c.x[q];
                    } else {
                        const I4 s = *reinterpret_cast<const I4*>(pool + t.at + i0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = tile_x(s.x[q]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int o = o0 + q;
                        if (o < lo || o >= hi) continue;
                        const long long i = loop ? mix_loop_index(base, o, t.len) : base + o;
                        v[q] = (t.flags & kMixClip) ? A.bank[t.at + i] : tile_x(pool[t.at + i]);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = conv_step(acc[q], v[q], gain);
            }
        }
        conv_stage4<F32>(staged, acc, o0, live);
        __syncthreads();
        tile_store<T>(A.tile.out, row.dst + t0, n, staged, tid);
        __syncthreads();      // `staged` is the next tile's
    }
}

}  // namespace klatt
#endif
