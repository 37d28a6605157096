// klatt_response.h -- the vocal-tract frequency response of a set batch (speechPlayer_batch_exportResponse) and of plain frames
// (speechPlayer_frameResponse).
//
// The filter network the synthesiser configures on every sample -- the cascade branch N0, NP, r6 .. r1 and the parallel branch p1 .. p6
// with parallelBypass (reference src/speechWaveGenerator.cpp:139-182) -- evaluated on the unit circle for the frame
// speechPlayer_batch_exportTracks defines for a sample: the frozen-time response of cur(t).  The definition is in
// include/speechPlayer_batch.h; this header is its one statement in code.  response_bin / response_kind are compiled for the host
// (speechPlayer_frameResponse) and for the device (klatt_response) from the same source, with -ffp-contract=off: every operation is
// a separately rounded binary64 operation on both, divisions and square roots are IEEE, and the twiddles of a bin are made once, on
// the host, for both.  The coefficients are the synthesiser's: coefficient_finish(coefficient_parts(f, bw)) on the device, and on the
// host the same fast_exp / fast_cos of klatt_math.h (the device's wave-uniform short cuts return their bits).
//
//   klatt_response   Rows that speak the same frame list have the same response, so the export's rows are taken in GROUPS, one per
//                    distinct list, and a group's response is computed once and stored to each of its rows (measured: the arithmetic,
//                    not the stores, binds: profiles/response_export.txt).  A workgroup of 256 lanes takes kRespSteps consecutive steps
//                    of a group at a time.  Once per step, lane = (step, resonator): the request by bisection over TimelineReq, the
//                    closed form of the 38 columns the network reads (timeline_side / fade_value, as klatt_timeline_dense), the
//                    resonator's (a, b, c); 52 doubles per step into LDS.  Then the bin loop, lane = (step, EL consecutive bins): the
//                    14 transfer functions from LDS (lanes of one step read the same words: broadcasts), the two branches, and per
//                    kind and row one 16-byte store where the address allows (EL = 2 float64 or 4 float32 elements; else element by
//                    element), consecutive lanes on consecutive bins of a step's [kind][bin] block.  Nothing in the bin loop is
//                    indexed at run time but LDS.
#pragma once

#include <math.h>
#include <stdint.h>

#include "klatt_device.h"
#include "klatt_timeline.h"

namespace klatt {

constexpr int kRespKinds = 8;               // SPEECHPLAYER_RESPONSE_KINDS
constexpr int kRespMaxBins = 4096;
constexpr int kRespSteps = 16;              // steps a workgroup prepares at a time (16 lanes each)
constexpr int kRespRowTile = 256;           // rows of a group whose first steps are staged in LDS at a time (a larger group repeats the bin loop)
// a step's values: (a, b, c) of resonator r at 3 r (the order of kResF: N0, NP, c6 .. c1, p1 .. p6), then the gains
constexpr int kRespCaNP = 42, kRespPa = 43, kRespBypass = 49, kRespPreGain = 50, kRespOutGain = 51, kRespVals = 52;
constexpr int kRespGains = 10;
// the frame parameters of the gains, in the order of the values 42 .. 51: caNP, pa1 .. pa6, parallelBypass, preFormantGain, outputGain
__device__ constexpr int kRespGainParam[kRespGains] = {23, 37, 38, 39, 40, 41, 42, 43, 44, 45};
static const int kRespGainParamHost[kRespGains] = {23, 37, 38, 39, 40, 41, 42, 43, 44, 45};
static const int kRespResF[kNumRes] = {13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30};      // kResF / kResB for the host
static const int kRespResB[kNumRes] = {21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36};

#define KLATT_RESP_HD __host__ __device__ __forceinline__

struct Cx { double re, im; };

KLATT_RESP_HD Cx cx_mul(Cx x, Cx y)
{
    Cx o;
    o.re = x.re * y.re - x.im * y.im;
    o.im = x.re * y.im + x.im * y.re;
    return o;
}

// a / (1 - b z1 - c z2) with z1 = c1 - i s1, z2 = c2 - i s2; zero for a == 0 (the resonator is silent from a fresh state: b p1 + c p2
// of zero memories).  D = (1 - b c1 - c c2) + i (b s1 + c s2); a / D = (a / |D|^2) conj(D), one IEEE division.
KLATT_RESP_HD Cx response_pole(double a, double b, double c, double c1, double s1, double c2, double s2)
{
    const double dr = 1.0 - b * c1 - c * c2;
    const double di = b * s1 + c * s2;
    const double q = a / (dr * dr + di * di);
    Cx o;
    o.re = q * dr;
    o.im = -(q * di);
    if (a == 0.0) { o.re = 0.0; o.im = 0.0; }
    return o;
}

// a + b z1 + c z2: the anti-resonator, always in FIR form (with cfN0 == 0 the coefficients are the non-inverted ones)
KLATT_RESP_HD Cx response_zero(double a, double b, double c, double c1, double s1, double c2, double s2)
{
    Cx o;
    o.re = a + b * c1 + c * c2;
    o.im = -(b * s1 + c * s2);
    return o;
}

// The two branches of one step at one bin.  V: the step's kRespVals values; (c1, s1, c2, s2): the bin's twiddles.
//   C = 0.5 (1 + (H_N0 H_NP - 1) caNP) H_6 H_5 H_4 H_3 H_2 H_1         (reference :148-156)
//   S = sum_k (H_pk - 1) pa_k,  P = 0.5 (S + (1 - S) parallelBypass)     (:171-179)
KLATT_RESP_HD void response_bin(const double* V, double c1, double s1, double c2, double s2, bool gain, bool needC, bool needP, Cx& C, Cx& P)
{
    C.re = 0.0; C.im = 0.0; P.re = 0.0; P.im = 0.0;
    if (needC) {
        const Cx n0 = response_zero(V[0], V[1], V[2], c1, s1, c2, s2);
        const Cx np = response_pole(V[3], V[4], V[5], c1, s1, c2, s2);
        const Cx t = cx_mul(n0, np);
        const double ca = V[kRespCaNP];
        Cx x;
        x.re = (1.0 + (t.re - 1.0) * ca) * 0.5;
        x.im = (t.im * ca) * 0.5;
#pragma unroll
        for (int r = 2; r < 8; ++r) x = cx_mul(x, response_pole(V[3 * r], V[3 * r + 1], V[3 * r + 2], c1, s1, c2, s2));
        C = x;
    }
    if (needP) {
        Cx s; s.re = 0.0; s.im = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int r = 8 + k;
            const Cx h = response_pole(V[3 * r], V[3 * r + 1], V[3 * r + 2], c1, s1, c2, s2);
            const double pa = V[kRespPa + k];
            s.re = s.re + (h.re - 1.0) * pa;
            s.im = s.im + h.im * pa;
        }
        const double bp = V[kRespBypass];
        P.re = (s.re + (1.0 - s.re) * bp) * 0.5;
        P.im = (s.im + (0.0 - s.im) * bp) * 0.5;
    }
    if (gain) {
        const double g = V[kRespPreGain] * V[kRespOutGain];
        C.re = C.re * g; C.im = C.im * g; P.re = P.re * g; P.im = P.im * g;
    }
}

// kind 0 .. 7: real part, imaginary part, magnitude, 20 log10 magnitude of the cascade (0 .. 3) or the parallel branch (4 .. 7)
KLATT_RESP_HD double response_kind(int kind, Cx C, Cx P)
{
    const Cx x = kind < 4 ? C : P;
    const int what = kind & 3;
    if (what == 0) return x.re;
    if (what == 1) return x.im;
    const double mag = sqrt(x.re * x.re + x.im * x.im);
    if (what == 2) return mag;
    return 20.0 * log10(mag);
}

// ---- the host's statement (speechPlayer_frameResponse; the twiddles of both entry points) -------------------------------------------
// w = 6.283185307179586 f / sr; (cos w, sin w, cos 2w, sin 2w) by libm, once per bin for the host and the device alike
inline void response_twiddles(double f, int sampleRate, double* tw)
{
    const double w = 6.283185307179586 * f / (double)sampleRate;
    tw[0] = cos(w); tw[1] = sin(w); tw[2] = cos(2.0 * w); tw[3] = sin(2.0 * w);
}

// coefficient_parts on the host: the same fast_exp / fast_cos inside their validated range (the device's short cuts for unreduced
// arguments return their bits: klatt_math.h), libm outside it, where the device calls its own library and the bits may differ
inline RadCos coefficient_parts_host(double f, double bw, double negPiOverSr, double twoPiOverSr)
{
    const double ex = negPiOverSr * bw;
    const double th = twoPiOverSr * -f;
    RadCos o;
    if (fabs(ex) <= 700.0 && fabs(th) <= 1.0e4) { o.rad = fast_exp(ex); o.cs = fast_cos(th); }
    else { o.rad = exp(ex); o.cs = cos(th); }
    return o;
}

// (a, b, c) of one resonator on the host: coefficient_finish(coefficient_parts(f, bw), anti, f), what speechPlayer_frameResponse and
// speechPlayer_resonatorCoefficients state
inline Coef resonator_coefficients_host(double f, double bw, bool anti, double negPiOverSr, double twoPiOverSr)
{
    const RadCos p = coefficient_parts_host(f, bw, negPiOverSr, twoPiOverSr);
    return coefficient_finish(p.rad, p.cs, anti, f);
}

// the kRespVals values of one frame (47 doubles)
inline void response_values_host(const double* frame, double negPiOverSr, double twoPiOverSr, double* V)
{
    for (int r = 0; r < kNumRes; ++r) {
        const double f = frame[kRespResF[r]], bw = frame[kRespResB[r]];
        const Coef k = resonator_coefficients_host(f, bw, r == 0, negPiOverSr, twoPiOverSr);
        V[3 * r] = k.a; V[3 * r + 1] = k.b; V[3 * r + 2] = k.c;
    }
    for (int g = 0; g < kRespGains; ++g) V[kRespCaNP + g] = frame[kRespGainParamHost[g]];
}

// ---- the device ---------------------------------------------------------------------------------------------------------------------
typedef float RespF32x4 __attribute__((ext_vector_type(4)));
typedef double RespF64x2 __attribute__((ext_vector_type(2)));

struct ResponseGroup {       // 48 B: the rows of an export that speak one frame list
    long long frame0;        // first frame of the list
    long long steps;         // ceil((L - phase) / hop), 0 when L <= phase
    long long span;          // steps the group writes per row: its steps (packed) or rowStride (padded: zeros past the end)
    long long chunk0;        // the group's first chunk of kRespSteps steps among all groups'
    long long rowAt;         // its rows' entries in rowBase
    uint32_t nFrames, nRows;
};
static_assert(sizeof(ResponseGroup) == 48, "ResponseGroup layout");

struct ResponseArgs {
    const double* frames;
    const TimelineReq* req;
    const ResponseGroup* groups;     // ascending chunk0, every group with at least one chunk
    long long nGroups, nChunks;
    const long long* rowBase;        // group after group: the first step of each row in the output
    long long hop, phase;
    const int* kinds;
    int nKinds;
    const double* tw;                // [K][4]
    int K;
    int gain, needC, needP;
    double negPiOverSr, twoPiOverSr;
    void* out;
};

// column `col` of cur(t) on the sample c samples after request R was dequeued (Rp: the request before it, when there is one):
// the closed form of klatt_timeline_dense, the same operations on the same operands
__device__ __forceinline__ double response_track(const double* __restrict__ frames, const TimelineReq& R, const TimelineReq& Rp, bool hasPrev,
                                                 long long c, int col)
{
    if (c == 0) {
        if (!hasPrev) return 0.0;
        return fade_value(timeline_side(frames, Rp.from, Rp.flags & 1u, col), timeline_side(frames, Rp.to, Rp.flags & 2u, col), 1.0);
    }
    const double ratio = c <= (long long)R.fade ? (double)c / (double)R.fade : 1.0;
    return fade_value(timeline_side(frames, R.from, R.flags & 1u, col), timeline_side(frames, R.to, R.flags & 2u, col), ratio);
}

template <bool F32>
__global__ void __launch_bounds__(256) klatt_response(const ResponseArgs A)
{
    constexpr int EL = F32 ? 4 : 2;
    __shared__ double vals[kRespSteps][kRespVals];
    __shared__ int live[kRespSteps];
    __shared__ long long bases[kRespRowTile];
    const int tid = threadIdx.x;
    const int K = A.K, nKinds = A.nKinds;
    const uint32_t groups = (uint32_t)(K + EL - 1) / EL;      // lanes per step in the bin loop
    for (long long chunk = blockIdx.x; chunk < A.nChunks; chunk += gridDim.x) {
        long long glo = 0, ghi = A.nGroups;                                          // the last group that begins on or before the chunk
        while (ghi - glo > 1) { const long long mid = (glo + ghi) >> 1; if (A.groups[mid].chunk0 <= chunk) glo = mid; else ghi = mid; }
        const ResponseGroup G = A.groups[glo];
        const long long j0 = (chunk - G.chunk0) * kRespSteps;
        // ---- once per step: lane = (step, resonator) ----
        {
            const int s = tid >> 4, r = tid & 15, rr = r < kNumRes ? r : kNumRes - 1;
            const long long j = j0 + s;
            bool valid = false;
            double f = 0.0, bw = 0.0, gv = 0.0;
            if (j < G.steps) {
                valid = true;
                const long long t = A.phase + j * A.hop;
                const TimelineReq* __restrict__ rq = A.req + G.frame0;
                long long lo = 0, hi = G.nFrames;                                   // the last request dequeued on or before t
                while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (rq[mid].first <= t) lo = mid; else hi = mid; }
                const TimelineReq R = rq[lo];
                const long long c = t - R.first;
                const bool hasPrev = lo > 0;
                TimelineReq Rp = R;
                if (c == 0 && hasPrev) Rp = rq[lo - 1];
                f = response_track(A.frames, R, Rp, hasPrev, c, kResF[rr]);
                bw = response_track(A.frames, R, Rp, hasPrev, c, kResB[rr]);
                if (r < kRespGains) gv = response_track(A.frames, R, Rp, hasPrev, c, kRespGainParam[r]);
            }
            // (every lane evaluates, idle ones on zeros: the wave-uniform short cuts of coefficient_parts ballot over a full wavefront)
            const RadCos p = coefficient_parts(f, bw, A.negPiOverSr, A.twoPiOverSr);
            const Coef k = coefficient_finish(p.rad, p.cs, r == 0, f);
            if (r < kNumRes) { vals[s][3 * r] = k.a; vals[s][3 * r + 1] = k.b; vals[s][3 * r + 2] = k.c; }
            if (r < kRespGains) vals[s][kRespCaNP + r] = gv;
            if (r == 0) live[s] = valid ? 1 : 0;
        }
        __syncthreads();
        // ---- the bin loop: lane = (step, EL consecutive bins) ----
        const long long left = G.span - j0;
        const uint32_t nSteps = left < kRespSteps ? (uint32_t)left : (uint32_t)kRespSteps;
        const uint32_t items = nSteps * groups;
        const long long perStep = (long long)nKinds * K;
        for (uint32_t row0 = 0; row0 < G.nRows; row0 += kRespRowTile) {
            const uint32_t nRows = min(G.nRows - row0, (uint32_t)kRespRowTile);
            if (row0) __syncthreads();
            if ((uint32_t)tid < nRows) bases[tid] = A.rowBase[G.rowAt + row0 + tid] * perStep;
            __syncthreads();
            for (uint32_t it = tid; it < items; it += 256u) {
                const uint32_t s = it / groups, b0 = (it - s * groups) * EL;
                const double* __restrict__ V = vals[s];
                const bool on = live[s] != 0;
                Cx C[EL], P[EL];
#pragma unroll
                for (int i = 0; i < EL; ++i) {
                    const uint32_t b = min(b0 + (uint32_t)i, (uint32_t)K - 1u);
                    const double4 w = *reinterpret_cast<const double4*>(A.tw + (size_t)b * 4);
                    response_bin(V, w.x, w.y, w.z, w.w, A.gain != 0, A.needC != 0, A.needP != 0, C[i], P[i]);
                }
                const long long at = (j0 + s) * perStep + b0;
                const bool whole = b0 + EL <= (uint32_t)K;
                for (int q = 0; q < nKinds; ++q) {
                    const int kind = A.kinds[q];
                    double v[EL];
#pragma unroll
                    for (int i = 0; i < EL; ++i) v[i] = on ? response_kind(kind, C[i], P[i]) : 0.0;
                    for (uint32_t row = 0; row < nRows; ++row) {
                        // (the 16-byte stores are non-temporal: the output is written once and read by another kernel, and left to itself
                        // the compiler splits a plain vector store to merge it with the element stores of the other path)
                        const long long e = bases[row] + at + (long long)q * K;
                        if (F32) {
                            float* o = static_cast<float*>(A.out) + e;
                            if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0)
                                __builtin_nontemporal_store(RespF32x4{(float)v[0], (float)v[1], (float)v[EL - 2], (float)v[EL - 1]}, reinterpret_cast<RespF32x4*>(o));
                            else {
#pragma unroll
                                for (int i = 0; i < EL; ++i) if (b0 + i < (uint32_t)K) o[i] = (float)v[i];
                            }
                        } else {
                            double* o = static_cast<double*>(A.out) + e;
                            if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) __builtin_nontemporal_store(RespF64x2{v[0], v[1]}, reinterpret_cast<RespF64x2*>(o));
                            else {
#pragma unroll
                                for (int i = 0; i < EL; ++i) if (b0 + i < (uint32_t)K) o[i] = v[i];
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace klatt
