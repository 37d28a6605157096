// klatt_filter.h -- a batch's PCM through cascades of second-order (biquad) recursive sections (speechPlayer_batch_exportFiltered) and
// plain PCM filtered on the host (speechPlayer_pcmFilter).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_RES_HD are
// compiled for the host and for the device from the same source: the input conversion (tile_x of klatt_tiles.h), the section
// (filter_section: transposed direct form II, five correctly rounded binary32 operations, the fused ones written __builtin_fmaf so that
// they are fused whatever the contraction flag says and exact on the host whatever the build flags), the closing y + 0.0f
// (filter_finish) and the int16 conversion (res_int16 of klatt_resample.h).
//
//   The plan        filter_plan: the sections of all filters back to back with their starts, a1 and a2 negated once, and the refusals
//                   (messages without the entry point's prefix).
//   The statement   filter_host: the states +0, then for every sample n = 0 .. L + tail - 1 ascending x = tile_x(s(n)) (+0 for n >= L),
//                   through sections 0 .. K-1 in order (the y of one is the x of the next), then filter_finish.
//   The lemma       Appending or inserting an identity section (b0 1, the rest 0) changes no output bit: its y = fmaf(1, x, s1) with
//                   s1 a zero is x except possibly in the sign of a zero; t = fmaf(0, x, s2), s1 = fmaf(-0, y, t), v = 0 x and
//                   s2 = fmaf(-0, y, v) are zeros while x is finite, so its states stay zeros; the sign of a zero operand never changes
//                   a nonzero result of the sections downstream (a product with a zero is a zero, a zero added to a nonzero value
//                   returns it), so two such runs agree everywhere except possibly in the signs of zeros; and filter_finish's + 0.0f
//                   makes a zero +0.  This is what lets a wavefront pad rows with fewer sections up to its bucket.
//   The packing     filter_pack: the rows ordered by bucket, then by outputs descending, cut into groups of kFilterLanes -- a wavefront
//                   each.  A group's rows are padded to kFilterLanes with rows of no sections, which read and write nothing; every
//                   row keeps its own first element in the output, so the output order is the caller's whatever the packing.
//                   tests/native/check_filter_pack.cpp holds it to its properties.
//   klatt_filter    One wavefront (a workgroup of 64 lanes) per group; lane r takes row r of the group and keeps the row's
//                   coefficients (5 per section) and states (2 per section) in registers from the first sample to the last.  Time is
//                   walked in tiles of kFilterTile samples.  A tile of the 64 rows is loaded row by row, consecutive lanes taking
//                   consecutive samples (256 or 128 contiguous bytes per load, masked by tile_inside, whatever the row's first
//                   element is; the row's start and extent come from the lane that owns it by v_readlane, so no load waits for
//                   another), into registers; it is written converted (tile_x) into the wavefront's LDS region at a row pitch of
//                   kFilterTile + 1 dwords, so that lane r reads element [r][t] without bank conflicts (bank (r + t) mod 64).  The
//                   next tile's loads are issued BEFORE the kFilterTile x K section steps of the current one and their values wait in
//                   registers (64 VGPRs) until the current tile has left: that is the double buffer, and it costs no second LDS
//                   region.  Samples outside, sections inside: one LDS read and one LDS write per sample whatever K is.  The outputs
//                   are staged IN PLACE -- lane r alone touches row r of the region, and element t is read before it is written -- in
//                   the output's type, +0 past the row's outputs, and leave through the row writer of klatt_tiles.h (tile_store_lane:
//                   16-byte stores where aligned, element stores at a run's ends), two (float32) or four (int16) rows per pass.  A
//                   padded row's remainder past the group's longest row is written from a zeroed region without any arithmetic.
//                   The workgroup is one wavefront, so __syncthreads() is a wavefront barrier and no wavefront waits for another.
//                   LDS: 64 x 65 x 4 = 16 640 bytes of samples + 1 024 of the rows' places in the output = 17 664 per wavefront;
//                   a CU's 160 KB hold nine.  Instantiated for K = 1, 2, 4, 8, 16 (filter_bucket) with the section loop unrolled.
//   Out of scope    Live handles and initial conditions in or out through this kernel (the state would have to persist across pulls:
//                   klatt_stage.h keeps it), NodePlayer, zero-phase (forward-backward) filtering, time-parallel (scan) formulations -- they cannot meet the sequential statement's
//                   bits --, and filling the chip with fewer than 64 x 1024 rows: a recursion cannot be cut in time bit-exactly.
//                   A row some value of which overflows is outside the bit-for-bit claim (it faults nothing).
#pragma once

#include <algorithm>
#include <vector>

#include "klatt_resample.h"

namespace klatt {

constexpr int kFilterMaxSections = 16;               // of one filter
constexpr long long kFilterMaxTable = 1ll << 16;     // sections of all filters of a call
constexpr long long kFilterMaxTail = 1ll << 20;      // extra outputs of zero input
constexpr int kFilterTile = 64;                      // consecutive samples of each row a wavefront takes at a time
constexpr int kFilterLanes = 64;                     // rows of a group: a lane each
constexpr int kFilterPitch = kFilterTile + 1;        // dwords between rows of the LDS region

static_assert(kFilterTile == kFilterLanes, "a load takes 64 consecutive samples of one row, a lane each");

// One section as the kernel and the statement hold it: a0 = 1, na1 = -a1, na2 = -a2
struct FilterSection { float b0, b1, b2, na1, na2; };
constexpr FilterSection kFilterIdentity{1.0f, 0.0f, 0.0f, -0.0f, -0.0f};

// One sample through one section: transposed direct form II, each line one correctly rounded binary32 operation.  Returns y.
KLATT_RES_HD float filter_section(const FilterSection& c, float x, float& s1, float& s2)
{
    const float y = __builtin_fmaf(c.b0, x, s1);
    const float t = __builtin_fmaf(c.b1, x, s2);
    s1 = __builtin_fmaf(c.na1, y, t);
    const float v = c.b2 * x;
    s2 = __builtin_fmaf(c.na2, y, v);
    return y;
}

// The closing + 0.0f: a zero of either sign becomes +0
KLATT_RES_HD float filter_finish(float y) { return y + 0.0f; }

// The instantiation a filter of K sections (1 .. 16) runs in: 1, 2, 4, 8 or 16, the rest identity sections (the lemma)
KLATT_RES_HD int filter_bucket(long long K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

// ---- the request, as every entry point plans it on the host -----------------------------------------------------------------------------
struct FilterPlan {
    long long nFilters = 0, tail = 0;
    std::vector<long long> start;              // [nFilters + 1]
    std::vector<FilterSection> sections;       // the filters back to back
};

// The plan of a request, or false with `why` set (without the entry point's prefix).  sections: float[nSections][5] = b0 b1 b2 a1 a2.
// filterOf (nRows entries; may be null) is checked by filter_row, row by row.
inline bool filter_plan(FilterPlan& P, const float* sections, const long long* secStart, long long nFilters, long long tail, std::string& why)
{
    char buf[240];
    static const char* const names[5] = {"b0", "b1", "b2", "a1", "a2"};
    if (tail < 0 || tail > kFilterMaxTail) { snprintf(buf, sizeof buf, "tail %lld (0 .. 2^20 extra outputs)", tail); why = buf; return false; }
    if (nFilters < 1) { snprintf(buf, sizeof buf, "%lld filters (at least 1)", nFilters); why = buf; return false; }
    if (!sections || !secStart) { why = "no filters (sections and secStart)"; return false; }
    if (secStart[0] != 0) { snprintf(buf, sizeof buf, "secStart[0] = %lld (the first filter starts at 0)", secStart[0]); why = buf; return false; }
    for (long long j = 0; j < nFilters; ++j) {
        const long long a = secStart[j], b = secStart[j + 1];
        if (b - a < 1 || b - a > kFilterMaxSections) { snprintf(buf, sizeof buf, "filter %lld has %lld sections (1 .. %d)", j, b - a, kFilterMaxSections); why = buf; return false; }
        if (b > kFilterMaxTable) { snprintf(buf, sizeof buf, "the filters have more than %lld sections in all", kFilterMaxTable); why = buf; return false; }
    }
    for (long long j = 0; j < nFilters; ++j)
        for (long long k = secStart[j]; k < secStart[j + 1]; ++k) {
            const float* c = sections + 5 * k;
            for (int q = 0; q < 5; ++q)
                if (!(fabsf(c[q]) <= 3.4028234663852886e38f)) {      // (a NaN fails the comparison)
                    snprintf(buf, sizeof buf, "%s of section %lld of filter %lld is %g (every coefficient is finite)", names[q], k - secStart[j], j, (double)c[q]);
                    why = buf; return false;
                }
            const double a1 = (double)c[3], a2 = (double)c[4];      // the pole test, in binary64 on the float32 values
            if (!(a2 < 1.0 && fabs(a1) < 1.0 + a2)) {
                snprintf(buf, sizeof buf, "section %lld of filter %lld has a1 = %.9g, a2 = %.9g: its poles are not strictly inside the unit circle (a2 < 1 and |a1| < 1 + a2)",
                         k - secStart[j], j, a1, a2);
                why = buf; return false;
            }
        }
    P.nFilters = nFilters; P.tail = tail;
    P.start.assign(secStart, secStart + nFilters + 1);
    P.sections.resize((size_t)secStart[nFilters]);
    for (size_t k = 0; k < P.sections.size(); ++k) {
        const float* c = sections + 5 * k;
        P.sections[k] = FilterSection{c[0], c[1], c[2], -c[3], -c[4]};
    }
    return true;
}

// The filter of row i, or -1 with `why` set
inline long long filter_row(const FilterPlan& P, const long long* filterOf, long long i, std::string& why)
{
    char buf[200];
    if (!filterOf) {
        if (P.nFilters == 1) return 0;
        snprintf(buf, sizeof buf, "no filterOf with %lld filters (NULL takes exactly 1)", P.nFilters); why = buf; return -1;
    }
    if (filterOf[i] < 0 || filterOf[i] >= P.nFilters) { snprintf(buf, sizeof buf, "filterOf[%lld] = %lld is not a filter (%lld)", i, filterOf[i], P.nFilters); why = buf; return -1; }
    return filterOf[i];
}

inline long long filter_length(long long L, long long tail) { return L + tail; }

// ---- the host's statement (speechPlayer_pcmFilter): the shared functions in a plain loop -------------------------------------------------
// format 1: out is float[Lout]; format 0: int16_t[Lout].  Returns Lout.  In: int16_t (PCM) or float (a signal's samples).
template <typename In>
inline long long filter_host(const In* pcm, long long length, const FilterSection* sec, long long K, long long tail, int format, void* out)
{
    const long long Lout = filter_length(length, tail);
    float s1[kFilterMaxSections], s2[kFilterMaxSections];
    for (long long j = 0; j < K; ++j) s1[j] = s2[j] = 0.0f;
    for (long long n = 0; n < Lout; ++n) {
        float x = n < length ? tile_x(pcm[n]) : 0.0f;
        for (long long j = 0; j < K; ++j) x = filter_section(sec[j], x, s1[j], s2[j]);
        res_store(out, format, n, filter_finish(x));
    }
    return Lout;
}

// ---- the packing ------------------------------------------------------------------------------------------------------------------------
// first element and samples of a row's input (the pool's utterance, a signal's row); its outputs; its first element in the output; its
// filter's first section and its sections (0: a group's filler, which reads and writes nothing)
struct FilterRow { long long src, len, outLen, dst, secAt, sections; };
// rows first .. first + kFilterLanes - 1 of the packed table; the group's instantiation; its longest output row and longest input row
struct FilterGroup { long long first, bucket, outMost, inMost; };

// The rows in the order the wavefronts take them: by bucket ascending, then by outLen descending (ties in the caller's order), cut
// into groups of kFilterLanes that hold one bucket each; `packed` holds kFilterLanes rows per group, fillers behind the last.
// (Row: FilterRow, or a row that carries more beside it -- klatt_stage.h; a filler is all zeros)
template <class Row>
inline void filter_pack(const std::vector<Row>& rows, std::vector<Row>& packed, std::vector<FilterGroup>& groups)
{
    std::vector<long long> order(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) order[i] = (long long)i;
    std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) {
        const int ba = filter_bucket(rows[(size_t)a].sections), bb = filter_bucket(rows[(size_t)b].sections);
        return ba != bb ? ba < bb : rows[(size_t)a].outLen > rows[(size_t)b].outLen;
    });
    packed.clear(); groups.clear();
    for (size_t at = 0; at < order.size();) {
        const int bucket = filter_bucket(rows[(size_t)order[at]].sections);
        FilterGroup g{(long long)packed.size(), bucket, 0, 0};
        int n = 0;
        for (; n < kFilterLanes && at < order.size() && filter_bucket(rows[(size_t)order[at]].sections) == bucket; ++n, ++at) {
            const Row& r = rows[(size_t)order[at]];
            packed.push_back(r);
            g.outMost = std::max(g.outMost, r.outLen);
            g.inMost = std::max(g.inMost, r.len);
        }
        for (; n < kFilterLanes; ++n) packed.push_back(Row{});
        groups.push_back(g);
    }
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct FilterArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const FilterRow* rows;               // the packed table
    const FilterGroup* groups;           // the groups of this launch's bucket
    long long nGroups;
    const FilterSection* sections;       // the filters back to back
    long long rowStride;                 // the padded form: a row's width
    void* out;
};

// Row q's value of what every lane holds for its own row: two v_readlane_b32 (q is a constant of the unrolled loops)
__device__ __forceinline__ long long filter_of_lane(long long v, int q)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, q);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), q);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The wavefront's loads of the tile at t0: row q's samples t0 .. t0 + kFilterTile - 1, a lane each, masked by tile_inside; nothing
// outside a row is loaded.  The lane's own row starts at `src` and has `len` samples.
template <typename In>
__device__ __forceinline__ void filter_load_rows(In (&next)[kFilterLanes], const In* __restrict__ in, long long src, long long len, long long t0, int lane)
{
    const long long left = len - t0, first = src + t0;
    const int mine = (int)(left < 0 ? 0 : left < kFilterTile ? left : kFilterTile);      // the lane's row has this many samples in the tile
#pragma unroll
    for (int q = 0; q < kFilterLanes; ++q) {
        const int has = __builtin_amdgcn_readlane(mine, q);
        const In* __restrict__ x = in + filter_of_lane(first, q);
        next[q] = tile_inside(lane, has) ? x[lane] : (In)0;
    }
}

// The wavefront's stores of the tile at t0: row q of the group has its values staged at region + q kFilterPitch dwords, its first
// element in the output (-1: a filler) and its outputs in where[q]
template <typename T>
__device__ __forceinline__ void filter_store_rows(void* out, const long long (*where)[2], long long rowStride, long long t0, const float* region, int lane)
{
    constexpr int PER = sizeof(T) == 4 ? 32 : 16;      // lanes a row takes: its kFilterTile elements touch at most 17 (float32) or 9 (int16) aligned 16 bytes
    static_assert(kFilterTile / kTileLane<T> + 1 <= PER, "a row's run fits its lanes");
    const int mis = tile_mis<T>(out), sub = lane / PER, i = lane % PER;
    for (int q0 = 0; q0 < kFilterLanes; q0 += kFilterLanes / PER) {
        const int q = q0 + sub;
        const long long dst = where[q][0], outLen = where[q][1];
        if (dst < 0) continue;
        const int n = tile_n(rowStride, outLen, t0, kFilterTile);
        if (n <= 0 || i >= tile_lanes<T>(mis, dst + t0, n)) continue;
        tile_store_lane(static_cast<T*>(out), mis, dst + t0, n, reinterpret_cast<const T*>(region + q * kFilterPitch), i);
    }
}

template <int K, bool F32, typename In = int16_t>
__global__ void __launch_bounds__(kFilterLanes) klatt_filter(const FilterArgs A)
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
        const FilterRow me = A.rows[G.first + lane];
        FilterSection c[K];
        float s1[K], s2[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            c[j] = j < me.sections ? A.sections[me.secAt + j] : kFilterIdentity;
            s1[j] = s2[j] = 0.0f;
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
                const long long live = me.outLen - t0;             // outputs of the tile inside the lane's row; the rest is padding
                for (int t = 0; t < TILE; ++t) {
                    float x = mine[t];
#pragma unroll
                    for (int j = 0; j < K; ++j) x = filter_section(c[j], x, s1[j], s2[j]);
                    staged[t] = t < live ? res_value<F32>(filter_finish(x)) : (T)0;
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
        __syncthreads();                                           // the last tile has left before the next group's first
    }
}

}  // namespace klatt
#endif
