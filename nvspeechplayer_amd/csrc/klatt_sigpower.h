// klatt_sigpower.h -- the power of a row of a caller's signal (speechPlayer_signal_t): the fixed reduction shape the host and the device
// share, so that an SNR against a float32 row -- convolved, resampled speech -- is the same bits on both sides (klatt_mix.h: the mix onto
// a signal; speechPlayer_batch_exportPowerOf, speechPlayer_signalPower).  Function bodies compiled for the host (plain C++17) and for the
// device from one source; tests/native/check_signal_power.cpp holds the index functions to brute force under the sanitizers.
//
// The definition.  For a row of L samples:
//   int16      (format 0) the pool's: S = sum s^2 as an exact unsigned 64-bit integer -- order-free -- and P = mix_power(S, L)
//              (klatt_mix.h).  The pool handed back as an int16 signal gives the pool's bits.
//   float32    (format 1) sq(x) = (double)x * (double)x.  The product of two binary32 values is EXACT in binary64 (24 + 24 significant
//              bits fit 53, and under the value bound no exponent leaves the range): whether the compiler fuses it into an FMA with
//              the addition that follows changes no bit, whatever the contraction flag says.  Samples at index L or beyond are +0.
//   block      kSigPowerBlock = 2048 consecutive samples, 256 LEAVES of kSigPowerLeaf = 8 consecutive samples.
//              leaf  = ((((((sq0 + sq1) + sq2) + sq3) + sq4) + sq5) + sq6) + sq7, ascending (sig_leaf);
//              block sum = the balanced binary tree over the 256 leaves in natural order, t[i] = t[2i] + t[2i+1], eight levels
//              (sig_tree).  On the device the first six levels are the xor butterfly d = 1, 2, .., 32 within a wavefront (binary64
//              addition is commutative: both lanes of a pair get the same bits, so every lane ends with the tree's value over its
//              wavefront's 64 leaves), and the four wave sums close the tree as (w0 + w1) + (w2 + w3) (sig_waves).
//   row        Q = the ascending sum of the block sums from +0.0; P = Q / (double)L, and P = 0 for L = 0 (sig_row_power).
//   Lemma      Every addend is >= +0: a square is, and a sum of such is.  x + (+0) = x bit for bit for every binary64 x >= +0 (+0
//              included: +0 + +0 = +0).  So absent samples, absent leaves, the absent part of a short last block and absent blocks
//              may be TAKEN AS ZEROS, or left out where the tree's shape allows, without changing a bit: the kernel never loads past
//              a row to "fill" a leaf, a lane whose leaf lies beyond the row adds +0 without touching memory, and the row pass may
//              add +0 for a lane that has no partial.
//   bound      The signal contract's (klatt_tiles.h): finite samples of magnitude at most 2^16, rows of at most 2^44 samples: a square
//              is at most 2^32, Q at most 2^76 -- no sum overflows.  Outside the bound the bits are unspecified; no sample's value
//              ever steers an address.
//   Both definitions are WHOLE-SIGNAL mean squares, silences included, as the pool's is.
// Why a tree and not exact accumulation: an exact (order-free) sum of binary64 squares needs a superaccumulator of some 2100 bits per
// row, or sorting by exponent -- neither fits a lane's registers nor one pass at the memory's rate; a fixed shape costs what any
// reduction costs and its error, 16 + nBlocks roundings, is far below what the float32 gain keeps.
//
//   The indices          sig_blocks, sig_leaf_start, sig_leaf_live, sig_leaf_whole: what a lane of the kernel visits.
//   The statement        sig_power_host: the definition in a plain loop over the shared functions.
//   klatt_signal_power   256 lanes per workgroup; a workgroup takes one block of one distinct row in a grid-stride walk over a table
//                        that counts BLOCKS (packed_locate).  Lane l owns leaf l: two 16-byte loads where the address is 16-byte aligned
//                        and the leaf lies wholly inside the row, masked scalars otherwise -- nothing outside 0 .. L-1 is loaded.  The
//                        butterfly, the four wave sums through LDS, one binary64 BLOCK PARTIAL per block into the call's scratch: no
//                        atomics, no order dependence.
//   klatt_signal_power_rows  a wavefront per distinct row: 64 partials at a time in one load, then the ascending chain over them by
//                        lane broadcasts, into one binary64 P per slot.
//   int16 signals        klatt_power's exact uint64 slots, turned into mix_power doubles by klatt_power_doubles (klatt_mix.h), so that
//                        everything downstream reads one array of binary64 powers per slot.
// The partials of one call take 8 bytes per 2048 powered samples in the call's staging slot; kSigPowerMaxBlocks = 2^24 of them (128 MB,
// 2^35 powered samples) is the most one call may ask for.
#pragma once

#include "klatt_tiles.h"

namespace klatt {

constexpr int kSigPowerLeaf = 8;                           // consecutive samples of a leaf
constexpr int kSigPowerLeaves = 256;                       // leaves of a block: a lane each
constexpr int kSigPowerBlock = 2048;                       // consecutive samples of one row a workgroup takes
constexpr long long kSigPowerMaxBlocks = 1ll << 24;        // block partials of one call

static_assert(kSigPowerBlock == kSigPowerLeaf * kSigPowerLeaves && kSigPowerLeaves == 4 * 64, "a leaf per lane, four wavefronts");

// ---- the definition's functions, host and device from one source ---------------------------------------------------------------------------
KLATT_RES_HD double sig_sq(float x) { return (double)x * (double)x; }

KLATT_RES_HD double sig_leaf(const float (&v)[kSigPowerLeaf])
{
    double acc = sig_sq(v[0]) + sig_sq(v[1]);
    for (int q = 2; q < kSigPowerLeaf; ++q) acc = acc + sig_sq(v[q]);
    return acc;
}

// The four wave sums of a block, in the tree's order
KLATT_RES_HD double sig_waves(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }

// ---- the kernel's index arithmetic ---------------------------------------------------------------------------------------------------------
KLATT_RES_HD long long sig_blocks(long long L) { return (L + kSigPowerBlock - 1) / kSigPowerBlock; }
// The first sample of leaf `leaf` of block j
KLATT_RES_HD long long sig_leaf_start(long long j, int leaf) { return j * kSigPowerBlock + (long long)leaf * kSigPowerLeaf; }
// Of the leaf's eight samples from s0, those inside the row: the first `live`
KLATT_RES_HD int sig_leaf_live(long long s0, long long L) { const long long left = L - s0; return (int)(left < kSigPowerLeaf ? (left > 0 ? left : 0) : kSigPowerLeaf); }
// The leaf at p lies wholly inside the row and p is 16-byte aligned: two 16-byte loads take it
KLATT_RES_HD bool sig_leaf_whole(const float* p, int live) { return live == kSigPowerLeaf && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the host's statement ------------------------------------------------------------------------------------------------------------------
// The tree over a block's 256 leaves, in place
inline double sig_tree(double (&t)[kSigPowerLeaves])
{
    for (int n = kSigPowerLeaves / 2; n >= 1; n /= 2)
        for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
}

// The sum of block j of a row of L samples: samples at L or beyond are +0
inline double sig_block_host(const float* x, long long L, long long j)
{
    double t[kSigPowerLeaves];
    for (int leaf = 0; leaf < kSigPowerLeaves; ++leaf) {
        const long long s0 = sig_leaf_start(j, leaf);
        float v[kSigPowerLeaf];
        for (int q = 0; q < kSigPowerLeaf; ++q) v[q] = s0 + q < L ? x[s0 + q] : 0.0f;
        t[leaf] = sig_leaf(v);
    }
    return sig_tree(t);
}

KLATT_RES_HD double sig_row_power(double Q, long long L) { return L > 0 ? Q / (double)L : 0.0; }

inline double sig_power_host(const float* x, long long L)
{
    double Q = 0.0;
    for (long long j = 0; j < sig_blocks(L); ++j) Q = Q + sig_block_host(x, L, j);
    return sig_row_power(Q, L);
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct PowerJob { long long src, len; };      // the first element (of the pool, of a signal's data) and the samples of a slot's row

struct SigPowerArgs {
    const float* data;
    const PowerJob* jobs;
    const long long* blockStart;      // [nJobs + 1] the first block of every job
    long long nJobs, nBlocks;
    double* partials;                 // [nBlocks]
};

// Six levels of the tree: every lane ends with the sum over its wavefront's 64 leaves (the 64-bit halves shuffled as power_wave_sum does)
__device__ __forceinline__ double sig_wave_sum(double v)
{
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = __shfl_xor((unsigned)u, d, 64), hi = __shfl_xor((unsigned)(u >> 32), d, 64);
        v = v + __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    return v;
}

__global__ void __launch_bounds__(256) klatt_signal_power(const SigPowerArgs A)
{
    __shared__ double waves[4];
    const int tid = threadIdx.x;
    for (long long g = blockIdx.x; g < A.nBlocks; g += gridDim.x) {
        long long r, j;
        packed_locate(g, A.blockStart, A.nJobs, r, j);      // (a job of no samples has no blocks: the last job that starts here is the one)
        const PowerJob job = A.jobs[r];
        const long long s0 = sig_leaf_start(j, tid);
        const int live = sig_leaf_live(s0, job.len);
        double leaf = 0.0;                                   // (the Lemma: a leaf beyond the row is +0, and nothing is loaded for it)
        if (live > 0) {
            const float* __restrict__ p = A.data + job.src + s0;
            float v[kSigPowerLeaf];
            if (sig_leaf_whole(p, live)) {
                const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            } else {
#pragma unroll
                for (int q = 0; q < kSigPowerLeaf; ++q) v[q] = q < live ? p[q] : 0.0f;
            }
            leaf = sig_leaf(v);
        }
        const double w = sig_wave_sum(leaf);
        if ((tid & 63) == 0) waves[tid >> 6] = w;
        __syncthreads();
        if (tid == 0) A.partials[g] = sig_waves(waves[0], waves[1], waves[2], waves[3]);
        __syncthreads();      // `waves` is the next block's
    }
}

// The row pass: slot r's partials blockStart[r] .. blockStart[r + 1] - 1 summed in ascending order from +0.0, over L.  A wavefront per
// slot: 64 partials in one load, ahead of the chain over them (lane k's value broadcast, k ascending); a lane without a partial holds +0
// (the Lemma).  Every lane of the wavefront carries the same chain.
__global__ void __launch_bounds__(256) klatt_signal_power_rows(const double* __restrict__ partials, const long long* __restrict__ blockStart,
                                                               const PowerJob* __restrict__ jobs, long long nJobs, double* __restrict__ powers)
{
    const int lane = threadIdx.x & 63;
    for (long long r = blockIdx.x * 4ll + (threadIdx.x >> 6); r < nJobs; r += gridDim.x * 4ll) {
        const long long b0 = blockStart[r], b1 = blockStart[r + 1];
        double Q = 0.0;
        for (long long at = b0; at < b1; at += 64) {
            const double mine = at + lane < b1 ? partials[at + lane] : 0.0;
            const unsigned long long u = (unsigned long long)__double_as_longlong(mine);
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const unsigned lo = __shfl((unsigned)u, k, 64), hi = __shfl((unsigned)(u >> 32), k, 64);
                Q = Q + __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
            }
        }
        if (lane == 0) powers[r] = sig_row_power(Q, jobs[r].len);
    }
}

}  // namespace klatt
#endif
