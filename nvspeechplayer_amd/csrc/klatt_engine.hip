// klatt_engine.hip -- host side of the MI355X Klatt engine and its C-ABI.
//
// Exports (include/speechPlayer.h, include/speechPlayer_batch.h):
//   the reference's five entry points  (reference src/speechPlayer.cpp:25-53)
//     -- each handle is a GPU-resident stream: queueFrame keeps the producer-side queue on the
//        host (as reference src/frame.cpp:90-115 does), synthesize runs the kernel for that one
//        stream from its saved state and copies the PCM back;
//   the additive batch entry points    (N independent streams per launch): setUtterances classifies the utterances, packs them
//     into wavefronts by length and timing and plans the tracks (plan_tracks); a synthesis call launches up to five groups side by
//     side (batch_launch) -- for speech: klatt_tracks, then the stage-parallel kernel with flat stages.
// There is no CPU synthesis path in this library: without a HIP device every entry point fails.
#include "klatt_device.h"
#include "klatt_systolic.h"
#include "klatt_lanepipe.h"
#include "klatt_tracks.h"
#include "klatt_direct.h"
#include "klatt_plan.h"
#include "klatt_timeline.h"
#include "klatt_align.h"
#include "klatt_source.h"
#include "klatt_response.h"
#include "klatt_stems.h"
#include "klatt_spectrum.h"
#include "klatt_resample.h"
#include "klatt_convolve.h"
#include "klatt_filter.h"
#include "klatt_codec.h"
#include "klatt_stage.h"
#include "klatt_stage_window.h"
#include "klatt_lpc.h"
#include "klatt_lpcsynth.h"
#include "klatt_pitch.h"
#include "klatt_stage_frames.h"
#include "klatt_tempo.h"
#include "klatt_mix.h"
#include "klatt_export.h"
#include "klatt_batchplan.h"
#include "klatt_hostpool.h"
#include "klatt_trackplan.h"
#include "klatt_live.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <atomic>
#include <system_error>
#include <thread>
#include <numeric>
#include <exception>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/speechPlayer_batch.h"

using namespace klatt;

// int16 PCM -> float in [-1, 1]: sample / 32767, the scaling of the reference's audio sink
// (reference lavPlayer.py:17).  HBM-bound elementwise pass: 8 samples (16 B) in, 32 B out per lane.
__global__ void __launch_bounds__(256) pcm_to_float(const int16_t* __restrict__ in, float* __restrict__ out, long long n8)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const uint4 v = reinterpret_cast<const uint4*>(in)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        float4 lo, hi;
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[2 * k] = (float)(int16_t)(w[k] & 0xFFFFu) / 32767.0f;
            f[2 * k + 1] = (float)(int16_t)(w[k] >> 16) / 32767.0f;
        }
        lo = make_float4(f[0], f[1], f[2], f[3]); hi = make_float4(f[4], f[5], f[6], f[7]);
        reinterpret_cast<float4*>(out)[2 * i] = lo;
        reinterpret_cast<float4*>(out)[2 * i + 1] = hi;
    }
}

// The PCM pool pads every utterance to a multiple of 32 samples (whole 64-byte row segments for the synthesis kernels' tile
// flushes); a consumer wants the utterances back to back.  pcm_compact writes that DENSE order in HBM, so that what crosses the
// link afterwards is ONE contiguous copy at the DMA engines' rate (until round 5 a host thread compacted 16-MB bounce buffers:
// 16 GB/s of a 63 GB/s link).  A thread owns 8 dense samples (one aligned 16-byte store): it finds its utterance by bisection
// over the dense starts, and -- when the 8 samples lie in one utterance, i.e. practically always -- reads the two aligned 16-byte
// vectors that cover them in the pool and shifts (the dense start of an utterance is any sample, so source and destination are
// misaligned by an even number of bytes that is the same for every thread of the utterance).  HBM-bound: 2 B read + 2 B written per sample.
__global__ void __launch_bounds__(256) pcm_compact(const int16_t* __restrict__ pool, int16_t* __restrict__ dense, const UttDesc* __restrict__ utt,
                                                   const long long* __restrict__ denseStart, long long nUtt, long long total)
{
    const long long n8 = (total + 7) / 8;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n8; t += stride) {
        const long long p = t * 8;
        long long lo = 0, hi = nUtt;                     // the last utterance whose dense start is <= p
        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (denseStart[mid] <= p) lo = mid; else hi = mid; }
        long long u = lo;
        const long long d0 = denseStart[u], d1 = denseStart[u + 1];
        uint32_t w[4];
        if (p + 8 <= d1) {
            const long long src = utt[u].outStart + (p - d0);            // in samples; the pool start of an utterance is a multiple of 32
            const int k = (int)(src & 7) * 2;                               // byte offset within the aligned 16-byte vector
            const uint4* a = reinterpret_cast<const uint4*>(pool + (src - (src & 7)));
            const uint4 v0 = a[0];
            uint32_t x[8] = {v0.x, v0.y, v0.z, v0.w, 0u, 0u, 0u, 0u};
            if (k) { const uint4 v1 = a[1]; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w; }
            const int dw = k >> 2, half = k & 2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a0 = 0, a1 = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) if (dw == q) { a0 = x[j + q]; a1 = x[j + q + 1 < 8 ? j + q + 1 : 7]; }
                w[j] = half ? (a0 >> 16) | (a1 << 16) : a0;
            }
        } else {
            // the 8 samples straddle utterances (or run past the end): sample by sample
            uint32_t s16[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long long q = p + i;
                uint32_t v = 0;
                if (q < total) {
                    while (q >= denseStart[u + 1]) ++u;   // (utterances of zero samples are stepped over)
                    v = (uint16_t)pool[utt[u].outStart + (q - denseStart[u])];
                }
                s16[i] = v;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = s16[2 * j] | (s16[2 * j + 1] << 16);
        }
        reinterpret_cast<uint4*>(dense)[t] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// SourceRef of every frame (klatt_device.h): what a flat or direct source stage reads when the frame is dequeued.  The division is
// the reference's (endVoicePitch - voicePitch) / minFrameDuration (src/frame.cpp:98), an IEEE double division here as there; a NULL
// frame carries no pitch of its own.
__global__ void __launch_bounds__(256) klatt_source_refs(const double* __restrict__ frames, const FrameMeta* __restrict__ meta, SourceRef* __restrict__ out, long long nFrames)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nFrames; k += stride) {
        const FrameMeta m = meta[k];
        const bool isNullFrame = (m.flags & FRAME_NULL) != 0;
        const double g0 = isNullFrame ? 0.0 : frames[k * kNumParams], g46 = isNullFrame ? 0.0 : frames[k * kNumParams + 46];
        SourceRef r;
        r.pitch = g0;
        r.pitchInc = isNullFrame ? 0.0 : __ddiv_rn(g46 - g0, (double)m.minSamples);
        r.invFade = __ddiv_rn(1.0, (double)m.fadeSamples);
        r.userIndex = m.userIndex;
        r.flags = m.flags & FRAME_NULL;
        out[k] = r;
    }
}

// 64-bit digest of every utterance's PCM, computed where the PCM lives: sum over the utterance's samples of
// mix64(position, value).  A sum, so lanes and wavefronts may add their shares in any order; one wavefront per utterance,
// 16 B (8 samples) per lane and step.  HBM-bound read of the pool.  (Checks of full-size configurations compare digests
// instead of copying tens of GB of PCM to the host; tests/test_gpu_parity.py restates the formula in numpy.)
__host__ __device__ inline unsigned long long digest_mix(unsigned long long pos, unsigned int value16)
{
    unsigned long long x = (pos + 1ull) * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)value16 + 1ull) * 0xC2B2AE3D27D4EB4Full;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    return x;
}
__global__ void __launch_bounds__(256) pcm_digest(const int16_t* __restrict__ pcm, const UttDesc* __restrict__ utt,
                                                  const UttResult* __restrict__ result, unsigned long long* __restrict__ out, long long nUtt)
{
    const int lane = threadIdx.x & 63;
    const long long wavesPerGrid = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long u = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < nUtt; u += wavesPerGrid) {
        const long long base = utt[u].outStart;          // multiple of 32 samples: 16-B aligned
        const unsigned int n = result[u].produced;
        unsigned long long acc = 0;
        for (unsigned int i = (unsigned int)lane * 8u; i < n; i += 64u * 8u) {
            const uint4 v = *reinterpret_cast<const uint4*>(pcm + base + i);
            const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (i + (unsigned int)k < n) acc += digest_mix(i + (unsigned int)k, (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)acc, m, 64);
            const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(acc >> 32), m, 64);
            acc += ((unsigned long long)hi << 32) | lo;
        }
        if (lane == 0) out[u] = acc;
    }
}

// speechPlayer_batch_exportPcm: chosen utterances of the pool into a caller's device buffer, as int16 or as float (/ 32767, the
// scaling of pcm_to_float), in rows of `rowStride` elements zero-padded past each utterance's end (rowStride > 0) or back to back
// (rowStride == 0: row r starts at dstStart[r]; chunkRow[c] is the row that holds element c * kExportChunk, so that the bisection for a
// thread's row runs over the few rows of its chunk -- over all 65 536 rows of configs[2] it was 16 dependent loads per 8 elements, and
// the kernel ran at a third of its bandwidth).  A thread owns 8 OUTPUT elements, so its store is one aligned 16-byte (int16) or two
// 16-byte (float) stores whatever the row stride, when the buffer is 16-byte aligned (vecStore).  Inside a row the source is misaligned
// against the destination by the same even number of bytes for every thread of the row: the two aligned 16-byte loads and the shift
// of pcm_compact.  8 elements that straddle rows or an utterance's end go element by element.  HBM-bound: 2 B read, 2 or 4 B written.
struct ExportRow { long long src, len; };      // pool offset (a multiple of kTile) and samples of a row's utterance
constexpr int kExportChunkLog2 = 15;
template <bool FLOAT>
__global__ void __launch_bounds__(256) pcm_export(const int16_t* __restrict__ pool, void* __restrict__ out, const ExportRow* __restrict__ rows,
                                                  const long long* __restrict__ dstStart, const long long* __restrict__ chunkRow, long long nRows,
                                                  long long rowStride, long long total, int vecStore)
{
    const long long n8 = (total + 7) / 8;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n8; t += stride) {
        const long long p = t * 8;
        long long r, c0, width;          // p's row, its column there, the row's width
        if (rowStride > 0) {
            r = p / rowStride; c0 = p - r * rowStride; width = rowStride;
        } else {
            const long long c = p >> kExportChunkLog2;
            long long lo = chunkRow[c], hi = chunkRow[c + 1] + 1;      // the last row whose start is <= p
            while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (dstStart[mid] <= p) lo = mid; else hi = mid; }
            r = lo; c0 = p - dstStart[r]; width = dstStart[r + 1] - dstStart[r];
        }
        uint32_t s16[8];
        const ExportRow row = rows[r];
        if (p + 8 <= total && c0 + 8 <= width && c0 + 8 <= row.len) {
            const long long src = row.src + c0;
            const int k = (int)(src & 7) * 2;
            const uint4* a = reinterpret_cast<const uint4*>(pool + (src - (src & 7)));
            const uint4 v0 = a[0];
            uint32_t x[8] = {v0.x, v0.y, v0.z, v0.w, 0u, 0u, 0u, 0u};
            if (k) { const uint4 v1 = a[1]; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w; }
            const int dw = k >> 2, half = k & 2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a0 = 0, a1 = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) if (dw == q) { a0 = x[j + q]; a1 = x[j + q + 1 < 8 ? j + q + 1 : 7]; }
                const uint32_t w = half ? (a0 >> 16) | (a1 << 16) : a0;
                s16[2 * j] = w & 0xFFFFu; s16[2 * j + 1] = w >> 16;
            }
        } else if (p + 8 <= total && c0 + 8 <= width && c0 >= row.len) {
#pragma unroll
            for (int i = 0; i < 8; ++i) s16[i] = 0u;       // padding
        } else {
            // across rows, across an utterance's end, or past the end of the output: element by element
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long long q = p + i;
                uint32_t v = 0;
                if (q < total) {
                    long long rr, c;
                    if (rowStride > 0) { rr = q / rowStride; c = q - rr * rowStride; }
                    else { while (q >= dstStart[r + 1]) ++r; rr = r; c = q - dstStart[r]; }     // (rows of zero samples are stepped over)
                    const ExportRow e = rows[rr];
                    if (c < e.len) v = (uint16_t)pool[e.src + c];
                }
                s16[i] = v;
            }
        }
        if (FLOAT) {
            float f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = (float)(int16_t)s16[i] / 32767.0f;
            float* o = static_cast<float*>(out) + p;
            if (vecStore && p + 8 <= total) {
                reinterpret_cast<float4*>(o)[0] = make_float4(f[0], f[1], f[2], f[3]);
                reinterpret_cast<float4*>(o)[1] = make_float4(f[4], f[5], f[6], f[7]);
            } else {
                for (int i = 0; i < 8 && p + i < total; ++i) o[i] = f[i];
            }
        } else {
            int16_t* o = static_cast<int16_t*>(out) + p;
            if (vecStore && p + 8 <= total) {
                reinterpret_cast<uint4*>(o)[0] = make_uint4(s16[0] | (s16[1] << 16), s16[2] | (s16[3] << 16), s16[4] | (s16[5] << 16), s16[6] | (s16[7] << 16));
            } else {
                for (int i = 0; i < 8 && p + i < total; ++i) o[i] = (int16_t)s16[i];
            }
        }
    }
}

// Frames given in device memory (speechPlayer_batch_setUtterancesDevice): the rows of the frames that stand for the batch's distinct
// shapes, gathered for the one download the track planner needs (FrameSource).
__global__ void __launch_bounds__(256) klatt_gather_frames(const double* __restrict__ frames, const long long* __restrict__ idx, long long nRows, double* __restrict__ out)
{
    const long long n = nRows * kNumParams;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const long long r = e / kNumParams;
        out[e] = frames[idx[r] * kNumParams + (e - r * kNumParams)];
    }
}

namespace {

thread_local std::string g_lastError;
thread_local int g_lastErrorCode = 0;      // speechPlayer_lastErrorCode(): 0 after a call that succeeded

void set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_lastError = buf;
    if (g_lastErrorCode == 0) g_lastErrorCode = SPEECHPLAYER_ERR_ARGUMENT;
    fprintf(stderr, "[speechPlayer/hip] %s\n", buf);
}
void set_error_code(int code) { g_lastErrorCode = code; }
// every entry point that can fail starts with this: the code then describes THIS call
void begin_call() { g_lastErrorCode = 0; }

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_error_code(SPEECHPLAYER_ERR_HIP);                                           \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -1;                                                                      \
        }                                                                                   \
    } while (0)

template <typename T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
        cap = n;
        return 0;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
    }
};

// Is this host memory page-locked (from speechPlayer_hostAlloc, or registered by the caller with hipHostRegister)?  Copies to and
// from such memory are one DMA transfer at the link's rate and truly asynchronous; pageable memory goes through bounce buffers.
static bool is_pinned(const void* p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// one page-locked host block, grown on demand
struct PinnedBlock {
    void* ptr = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        release();
        HIP_TRY(hipHostMalloc(&ptr, bytes + bytes / 8, hipHostMallocDefault));
        cap = bytes + bytes / 8;
        return 0;
    }
    void release()
    {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr; cap = 0;
    }
};

// two pinned host buffers + events for pipelined device-to-host copies
struct PinnedPair {
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        release();
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(hipHostMalloc(&buf[i], bytes, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        cap = bytes;
        return 0;
    }
    void release()
    {
        for (int i = 0; i < 2; ++i) {
            if (buf[i]) (void)hipHostFree(buf[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            buf[i] = nullptr; ev[i] = nullptr;
        }
        cap = 0;
    }
};

// Raise a kernel's dynamic-LDS limit once per (kernel, device): the attribute is per device, and a process may
// drive several devices (one BatchPlayer each).
int ensure_lds_limit(const void* kernel, int ldsBytes)
{
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> done;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(mu);
    for (const auto& e : done)
        if (e.first == kernel && e.second == dev) return 0;
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ldsBytes));
    done.emplace_back(kernel, dev);
    return 0;
}

KernelArgs base_args(int sampleRate)
{
    KernelArgs a;
    memset(&a, 0, sizeof a);
    a.sampleRate = sampleRate;
    a.sampleRateF = (double)sampleRate;
    a.invSampleRate = 1.0 / (double)sampleRate;
    a.negPiOverSr = -M_PI / sampleRate;          // reference src/speechWaveGenerator.cpp:116
    a.twoPiOverSr = (M_PI * 2) / sampleRate;     // reference src/speechWaveGenerator.cpp:31,118
    a.maxSamples = 0xFFFFFFFFu;
    return a;
}

template <bool NOISE, int CH, int WPS = 1, bool NASAL = true, bool STREAM = false, bool FLAT = false, bool LONE = false>
int launch_systolic(const KernelArgs& a, int mode, long long nGroups, hipStream_t stream)
{
    if (nGroups <= 0) return 0;
    if (nGroups > 0x7FFFFFFF) { set_error("too many workgroups: %lld", nGroups); return -1; }
    constexpr int ldsBytes = SysLds<NOISE, CH, FLAT, stream_split<STREAM, WPS, LONE>()>::kBytes + (LONE ? kStages * kLoneLdsPerStage : 0);     // LONE: a stage's fade chunks pass through LDS
    static_assert(ldsBytes <= 160 * 1024, "a workgroup's LDS");
    auto go = [&](auto kernel) -> int {
        if (ensure_lds_limit(reinterpret_cast<const void*>(kernel), ldsBytes)) return -1;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nGroups), dim3(kLanes * kStages), ldsBytes, stream, a);
        return 0;
    };
    int rc;
    switch (mode) {
    case MODE_EXACT: rc = go(klatt_systolic<MODE_EXACT, NOISE, CH, WPS, NASAL, STREAM, FLAT, LONE>); break;
    case MODE_FAST: rc = go(klatt_systolic<MODE_FAST, NOISE, CH, WPS, NASAL, STREAM, FLAT, LONE>); break;
    default: set_error("unknown arithmetic mode %d", mode); return -1;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the direct stages (klatt_direct.h): eight wavefronts per workgroup; `lean`: two workgroups per CU (8-sample hand-overs, 77 KB of pipes,
// 128 registers per stage), else one (16-sample hand-overs, 152 KB, 256 registers)
constexpr int kDirectChunk = 16, kDirectLeanChunk = 8;
template <int CH, int WPE>
int launch_direct_as(const KernelArgs& a, int mode, long long nGroups, hipStream_t stream)
{
    constexpr int ldsBytes = DirectLds<CH>::kBytes;
    auto go = [&](auto kernel) -> int {
        if (ensure_lds_limit(reinterpret_cast<const void*>(kernel), ldsBytes)) return -1;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nGroups), dim3(kLanes * kDirectStages), ldsBytes, stream, a);
        return 0;
    };
    int rc;
    switch (mode) {
    case MODE_EXACT: rc = go(klatt_direct<MODE_EXACT, CH, WPE>); break;
    case MODE_FAST: rc = go(klatt_direct<MODE_FAST, CH, WPE>); break;
    default: set_error("unknown arithmetic mode %d", mode); return -1;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int launch_direct(const KernelArgs& a, int mode, bool lean, long long nGroups, hipStream_t stream)
{
    if (nGroups <= 0) return 0;
    if (nGroups > 0x7FFFFFFF) { set_error("too many workgroups: %lld", nGroups); return -1; }
    return lean ? launch_direct_as<kDirectLeanChunk, 4>(a, mode, nGroups, stream) : launch_direct_as<kDirectChunk, 2>(a, mode, nGroups, stream);
}

#ifndef KLATT_LP_CH
#define KLATT_LP_CH 32     // hand-over size of the lane-pipelined kernel with one workgroup per CU
#endif
template <int CH, int WPS>
int launch_lanepipe(const KernelArgs& a, int mode, long long nGroups, hipStream_t stream)
{
    if (nGroups <= 0) return 0;
    if (nGroups > 0x7FFFFFFF) { set_error("too many workgroups: %lld", nGroups); return -1; }
    constexpr int ldsBytes = LpLds<CH>::kBytes;
    auto go = [&](auto kernel) -> int {
        if (ensure_lds_limit(reinterpret_cast<const void*>(kernel), ldsBytes)) return -1;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nGroups), dim3(kLanes * kStages), ldsBytes, stream, a);
        return 0;
    };
    int rc;
    switch (mode) {
    case MODE_EXACT: rc = go(klatt_lanepipe<MODE_EXACT, CH, WPS>); break;
    case MODE_FAST: rc = go(klatt_lanepipe<MODE_FAST, CH, WPS>); break;
    default: set_error("unknown arithmetic mode %d", mode); return -1;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// Which kernel runs the batch's groups (64 utterances per group)?  Measured on MI355X:
// stage-parallel workgroups (klatt_systolic.h) win at every batch size and for both groups -- 2.8e11 samples/s
// at 65 536 steady vowels against 1.3e11 for the lane kernel, 28.8 ms against 37.1 ms on cfg2 -- so "auto"
// always takes them; the lane kernel stays selectable (layout 0) and runs the streaming handles.
// Quiet batches that fit one workgroup per CU use 32-sample hand-overs (fewer barriers), else 16.
#ifndef KLATT_NOISY_CH
#define KLATT_NOISY_CH 8
#endif
struct GroupPlan { bool systolic; int chunk; };
GroupPlan plan_group(int layout, bool noisy, long long nUttBatch, long long nNoisyBatch, int cus)
{
    const long long groups = (nUttBatch + kLanes - 1) / kLanes + 1;
    GroupPlan p;
    p.systolic = layout != 0;
    (void)nNoisyBatch;
    p.chunk = noisy ? (groups <= cus ? 16 : 8)      // noisy: 8-sample hand-overs fit two workgroups per CU (LDS 80 KB each)
                    : (groups <= cus ? 32 : 16);
    return p;
}

template <bool STREAM, bool NOISE>
int launch(const KernelArgs& a, int mode, long long nWaves, hipStream_t stream)
{
    if (nWaves <= 0) return 0;
    if (nWaves > 0x7FFFFFFF) { set_error("too many wavefronts: %lld", nWaves); return -1; }
    constexpr int ldsBytes = LdsLayout<STREAM>::kBytes;
    auto go = [&](auto kernel) -> int {
        if (ensure_lds_limit(reinterpret_cast<const void*>(kernel), ldsBytes)) return -1;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nWaves), dim3(kLanes), ldsBytes, stream, a);
        return 0;
    };
    int rc;
    switch (mode) {
    case MODE_EXACT: rc = go(klatt_synthesize<MODE_EXACT, STREAM, NOISE>); break;
    case MODE_FAST: rc = go(klatt_synthesize<MODE_FAST, STREAM, NOISE>); break;
    default:
        set_error("unknown arithmetic mode %d", mode);
        return -1;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int pick_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error_code(SPEECHPLAYER_ERR_NO_DEVICE);
        set_error("no HIP device available (%s); this engine has no CPU path", e == hipSuccess ? "count 0" : hipGetErrorString(e));
        return -1;
    }
    if (device < 0) {
        const char* env = getenv("SPEECHPLAYER_DEVICE");
        if (env) device = atoi(env);
        else if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n) { set_error("device %d out of range (%d devices)", device, n); return -1; }
    return device;
}

// ------------------------------------------------------------------------------------------
// Batch
// ------------------------------------------------------------------------------------------
struct Stage;
struct Batch {
    int sampleRate = 0;
    int device = 0;
    int mode = MODE_EXACT;
    int sortByLength = 1;
    int layout = -1;                       // -1: choose per group (plan_group); 2: lane-pipelined where eligible; 1: stage-parallel workgroups; 0: one wave per 64 utterances
    int cus = 256;
    hipStream_t stream = nullptr;
    int tracks = 1;                        // 1: noisy utterances with finite parameters run on flat stages fed by tracks (klatt_tracks.h)
    long long trackBudgetMB = 4096;        // the tracks of a batch may take this much device memory (at most 4 GB: the flat stages address them with 32-bit byte offsets); utterances beyond it run untracked
    hipStream_t side[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // the other groups run beside the last one (batch_launch)
    hipEvent_t forkEvent = nullptr, join[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int quietLast = 1;                     // option "quiet_last": the quiet groups are launched after the noisy ones (batch_launch)
    int deadTerms = 1;                     // option "dead_terms": a flat wavefront none of whose lanes has a term (UTT_TURBULENCE .. UTT_PARALLEL1) runs a body without it; 0: the general bodies
    DeviceBuffer<uint32_t> dDeadWaves;     // [3] the last tracked launch's wavefronts without parallel 1 / turbulence / the aspiration generator (speechPlayer_batch_kernelInfo),
                                           // then [kDead2Counts] without the nasal pair / parallel 5 / parallel 5 and 6 / parallel 1..4
    long long planDeadWaves[3] = {0, 0, 0};   // ... and what the plan says they will be (dead_wave_counts, klatt_batchplan.h): reported until the batch has been launched
    long long planDead2Waves[kDead2Counts] = {0, 0, 0, 0};   // (dead2_wave_counts)
    DeviceBuffer<uint32_t> dPresent2;      // [nUtt] the utterances' second word of present terms (UTT2_*): read by the flat launch alone
    long long nUtt = 0, nFrames = 0, nSlots = 0;   // nFrames: frames resident in HBM (the lists')
    long long nLists = 0, nFramesSpoken = 0;       // frame lists of the batch; frames the utterances queue (sum over utterances of their list's)
    std::vector<long long> uttFrameStart;          // [nUtt] first frame of the utterance's list
    std::vector<uint32_t> uttFrames;               // [nUtt] its number of frames
    bool launched = false;                         // a synthesis launch has been queued since the batch was set
    long long nQuiet = 0;                  // order[0..nQuiet) = utterances without noise, the rest with
    long long nTracked = 0;                // order[nQuiet..nQuiet + nTracked) = noisy utterances with tracks (slots: utterances + padding)
    long long nTrackedUtt = 0;             // the utterances among them
    long long nJobs = 0, trackEntries = 0; // distinct tracks of the batch, their entries (16 B each)
    int directLean = -1;                   // the direct stages' residency: 1 two workgroups per CU (the lean stages), 0 one, -1 the engine's choice (direct_lean())
    bool directAligned = false;            // of the resident batch's direct group (set_commit; false without one): half or more of the direct candidates sit in runs of 32 or more equally long, equally timed utterances
    int direct = 1;                        // noisy utterances with finite, bounded parameters and no tracks: 1 the direct stages (klatt_direct.h) unless their
                                           // lanes are time-aligned and the mode is MODE_EXACT (setUtterances), 2 the direct stages always, 0 the stages with the frame state machine
    long long nDirect = 0;                 // order[nQuiet + nTracked .. + nDirect) = such utterances (slots)
    long long nDirectUtt = 0, nDirectFrames = 0;
    long long nNoNasal = 0;                // order[0..nNoNasal) = quiet utterances that never couple the nasal pair (UTT_NO_NASAL); slots
    long long nNoNasalUtt = 0;             // the utterances among them (the rest: replicas that complete a sparse last wavefront)
    long long totalSamples = 0, poolSamples = 0;
    std::vector<uint32_t> lens;
    std::vector<uint32_t> uttSeed;     // [nUtt] the utterances' noise seeds (speechPlayer_batch_exportStems)
    std::vector<long long> outStart;   // padded offsets in the device pool
    std::vector<UttResult> results;
    bool resultsFresh = false;
    DeviceBuffer<double> dFrames;
    DeviceBuffer<FrameMeta> dMeta;
    DeviceBuffer<UttDesc> dUtt;
    DeviceBuffer<uint32_t> dOrder;
    DeviceBuffer<int16_t> dPcm;
    DeviceBuffer<UttResult> dResult;
    DeviceBuffer<FlatRef> dFlatRef;            // [nFrames] the same for the flat filter stages: one 16-byte load per fade start
    DeviceBuffer<SourceRef> dSourceRef;        // [nFrames] what the flat source stage reads at a dequeue
    DeviceBuffer<TrackJob> dJobs;
    DeviceBuffer<double> dShapes;              // [nShapes][kShapeStride]
    DeviceBuffer<double2> dTrack;
    DeviceBuffer<DirectJob> dDirectJobs;       // [nDirectFrames] the end points of every direct frame's fade (host walk of reference src/frame.cpp:55-72)
    DeviceBuffer<uint32_t> dDirectFirst;       // [nUtt] record number of an utterance's first frame
    DeviceBuffer<DirectHdr> dDirectHdr;        // [8][nDirectFrames] written by klatt_seeds in every launch
    DeviceBuffer<double2> dDirectRec;          // [kDirectEntries][nDirectFrames]
    DeviceBuffer<unsigned long long> dDebug;   // KLATT_STAMPS builds
    DeviceBuffer<float> dFloat;                // float copy of the PCM pool (speechPlayer_batch_readFloat)
    DeviceBuffer<unsigned long long> dDigest;  // per-utterance digests (speechPlayer_batch_digest)
    PinnedPair bounce;                         // speechPlayer_batch_readAll into pageable memory
    DeviceBuffer<FrameRecord> dRecords;        // speechPlayer_batch_setRecords: the records as they crossed the link (klatt_expand_frames reads them)
    DeviceBuffer<double> dShapeTable;          // ... and the call's shape table
    DeviceBuffer<uint32_t> dRep;               // klatt_verify_shared: per frame the frame the planner took its shape values from
    DeviceBuffer<unsigned long long> dMismatch;
    DeviceBuffer<FrameFacts> dFacts;           // klatt_frame_facts' output (frames that arrived by DMA are classified and hashed on the device)
    PinnedBlock hFacts;                        // ... and where it lands on the host
    DeviceBuffer<int16_t> dDense;              // the utterances back to back (pcm_compact): what speechPlayer_batch_readAll copies out
    DeviceBuffer<long long> dDenseStart;       // [nUtt + 1] dense start of every utterance (prefix sum of the closed-form lengths)
    std::vector<long long> denseStart;         // the same on the host
    hipStream_t copyStream = nullptr;          // device-to-host copies of dDense run here, beside the next launch on `stream`
    hipEvent_t denseReady = nullptr, copyDone = nullptr;
    bool copyPending = false;                  // a speechPlayer_batch_readAllAsync copy is in flight (speechPlayer_batch_readWait)
    bool floatFresh = false;
    // speechPlayer_batch_setUtterancesDevice: the caller's frames are ready on its stream when inputReady (recorded there) has passed;
    // the distinct shapes' rows the track planner reads (FrameSource) are gathered into dShapeRows and downloaded
    hipEvent_t inputReady = nullptr;
    DeviceBuffer<long long> dShapeIdx;
    DeviceBuffer<double> dShapeRows;
    // speechPlayer_batch_exportPcm runs on the CALLER's stream: behind pcmReady (recorded on `stream`, which every launch joins its side
    // streams into), with its rows staged through one of kExportSlots page-locked / device buffer pairs; a slot is reused once its `done`
    // (recorded behind its kernel) has passed, and every launch and set call makes `stream` wait for the slots' last exports
    hipEvent_t pcmReady = nullptr;
    struct ExportSlot { PinnedBlock host; DeviceBuffer<unsigned char> dev; hipEvent_t done = nullptr; bool used = false; };
    static constexpr int kExportSlots = 16;
    ExportSlot exportSlot[kExportSlots];
    unsigned exportNext = 0;
    // The exports of the batch AS SET (tracks, alignment and units, source and epochs, response, stems) share one path: "the export
    // path" below settle_track_exports says what they read, how they are ordered and what each of these members is for.
    struct SharedTable {                       // the order among the exports that share a table: each follows the one before on the device
        hipEvent_t done = nullptr;
        bool used = false;
        int wait(hipStream_t st) { if (used) HIP_TRY(hipStreamWaitEvent(st, done, 0)); return 0; }      // (whichever stream it ran on)
        int mark(hipStream_t st) { HIP_TRY(hipEventRecord(done, st)); used = true; return 0; }
    };
    std::vector<uint32_t> uttList;             // [nUtt] the list an utterance speaks
    DeviceBuffer<long long> dListStart;        // [nLists + 1]
    DeviceBuffer<TimelineReq> dTimeline;       // [nFrames] the per-request records, built once per set call by the first export
    hipEvent_t setDone = nullptr, setCopied = nullptr, timelineReady = nullptr;
    bool timelineFresh = false;
    ExportSlot trackSlot[kExportSlots];
    unsigned trackNext = 0;
    DeviceBuffer<double> dPitch;               // [slot][step] voicePitch of the lists a track export with column 0 speaks
    SharedTable pitchOrder;
    long long pitchBudgetMB = 256;             // option "pitch_table_mb": an export whose voicePitch table would be larger proceeds in pieces
    // klatt_align.h: the labels of a batch set with labels (one per list frame) and unitFirst[] (list l's entries from
    // listStart[l] + l), uploaded on the copy stream by the set call -- ahead of setCopied
    DeviceBuffer<FrameLabel> dLabels;
    DeviceBuffer<uint32_t> dUnitFirst;
    std::vector<uint32_t> listUnits;           // [nLists] units of a list
    bool hasLabels = false;
    // klatt_source.h: the step table and the epoch table follow one order; the per-list epoch counts are those of the batch as set,
    // kept until the next set call
    DeviceBuffer<double> dSource;              // [slot][step][6]
    DeviceBuffer<double> dEpochs;              // [epoch][4], list after list
    SharedTable sourceOrder;
    DeviceBuffer<long long> dEpochCount;       // [nLists] what the counting walk leaves
    std::vector<long long> epochCount;         // [nLists]
    bool epochFresh = false;
    long long sourceBudgetMB = 256;            // option "source_table_mb": an export whose step table would be larger proceeds in pieces
    long long sourceLaneLists = 12288;         // option "source_lane_lists": a walk over this many lists or more runs one lane per list
    // klatt_resample.h: the last request's plan and its table as the kernel reads it, kept until the parameters change; the exports that
    // read the table follow one order, so that an upload on one stream stands behind the readers on another
    ResPlan resPlan;
    DeviceBuffer<float> dResample;             // [taps][up]
    bool resOnDevice = false;
    SharedTable resampleOrder;
    // klatt_mix.h: the noise bank (speechPlayer_batch_setNoiseBank) -- the clips' starts and powers on the host, their samples on the
    // device -- kept across set calls until it is replaced; the exports that read it follow one order, which a replacement waits for
    MixBank bank;
    bool hasBank = false;
    DeviceBuffer<float> dBank;
    SharedTable bankOrder;
    // klatt_stage.h: the signal stages made on this batch; freed with it
    std::vector<Stage*> stages;
};

// ---- a signal stage (klatt_stage.h): the per-row state of one sequential export, fed chunk by chunk ---------------------------------------
// It belongs to a batch, which gives it the device, the staging blocks and the sixteen-in-flight slots.  The resampler's table is the
// stage's own, uploaded once when it is made: the batch's table follows the last whole-row request, and two stages at different rates on
// one batch would upload theirs again at every push.  Its pushes follow one another by `done`, whichever streams they are issued on.
struct Stage {
    Batch* b = nullptr;
    StageGeometry g;
    long long nRows = 0;
    std::vector<long long> N, M;               // [nRows] consumed and emitted since the row's start
    ResPlan res;                               // resample
    DeviceBuffer<float> dTable;                // [taps][up]
    DeviceBuffer<float> dHist[2];              // resample, convolution, spectrogram: the rows' histories, row r's from histAt[r] of either; dHist[cur] is what the next push reads
    int cur = 0;
    std::vector<long long> histAt;             // [nRows + 1] (all 0 where the kind keeps none)
    long long mostHistory = 0;                 // the longest row's
    FilterPlan fil;                            // filter
    std::vector<long long> secAt, secN;        // [nRows] the row's filter: its first section and its sections
    DeviceBuffer<float> dFilterState;          // [nRows][kStageFilterState]
    int codec = 0;                             // code
    DeviceBuffer<int> dCodeState;              // [nRows][2]
    std::vector<long long> irAt;               // convolution: [nRows] the row's response, its first tap (its taps: the row's history + 1)
    DeviceBuffer<float> dTaps;                 // the responses back to back
    SpecPlan spec;                             // spectrogram: the plan without its arrays, which the device holds
    DeviceBuffer<float> dWindow, dWeights;
    DeviceBuffer<SpecCx> dTw;
    DeviceBuffer<int> dRange;
    LpcPlan lpc;                               // LPC: the plan without its arrays, which the device holds (dWindow, dLag)
    DeviceBuffer<double> dLag;
    PitchPlan pitch;                           // pitch
    hipEvent_t done = nullptr;
    bool used = false;
};
std::mutex g_stageMutex;
std::vector<Stage*> g_stages;                  // every live stage: a handle that is not here was freed (or never made)

bool stage_known(Stage* s)
{
    std::lock_guard<std::mutex> lock(g_stageMutex);
    return std::find(g_stages.begin(), g_stages.end(), s) != g_stages.end();
}
// Frees a live stage: its last push first
void stage_release(Stage* s)
{
    {
        std::lock_guard<std::mutex> lock(g_stageMutex);
        g_stages.erase(std::remove(g_stages.begin(), g_stages.end(), s), g_stages.end());
    }
    if (s->b) {
        (void)hipSetDevice(s->b->device);
        auto& all = s->b->stages;
        all.erase(std::remove(all.begin(), all.end(), s), all.end());
    }
    if (s->done) { if (s->used) (void)hipEventSynchronize(s->done); (void)hipEventDestroy(s->done); }
    s->dTable.release(); s->dHist[0].release(); s->dHist[1].release(); s->dFilterState.release(); s->dCodeState.release();
    s->dTaps.release(); s->dWindow.release(); s->dWeights.release(); s->dTw.release(); s->dRange.release(); s->dLag.release();
    delete s;
}

// The batch's own streams wait (on the device) for the exports that still read its pool.
int wait_exports(Batch* b)
{
    for (auto& s : b->exportSlot)
        if (s.used) HIP_TRY(hipStreamWaitEvent(b->stream, s.done, 0));
    return 0;
}
// ... and the host, before the pool or a slot is freed.
int sync_exports(Batch* b)
{
    for (auto& s : b->exportSlot)
        if (s.used) { HIP_TRY(hipEventSynchronize(s.done)); s.used = false; }
    return 0;
}

// A set call replaces what the track exports read.  Where the buffers are reused its two streams wait for the exports in flight on the
// device; where one is freed (it must grow), or where the frames are copied outside the streams' order, the host waits.
int settle_track_exports(Batch* b, bool onHost)
{
    for (auto& s : b->trackSlot) {
        if (!s.used) continue;
        if (onHost) { HIP_TRY(hipEventSynchronize(s.done)); s.used = false; }
        else { HIP_TRY(hipStreamWaitEvent(b->stream, s.done, 0)); HIP_TRY(hipStreamWaitEvent(b->copyStream, s.done, 0)); }
    }
    return 0;
}

// ---- the export path ------------------------------------------------------------------------------------------------------------------
// Every export of the batch AS SET -- tracks, alignment and units, source and epochs, response, stems -- fills the caller's device
// memory on the CALLER's stream from what a set call leaves resident: the frames, the meta words, the list table and (a batch with
// labels) the labels.  It is ordered by events only: behind the set call's own device work (setDone, setCopied: recorded by the set
// call on its two streams), behind the per-request records (built once per set call, by the first export: timelineReady, recorded
// behind klatt_timeline_requests on that export's stream) and ahead of the NEXT set call, which waits for the slots' last exports
// before it overwrites what they read (settle_track_exports).  What its kernels need beside the batch -- columns, rows, row tables,
// list descriptors -- crosses the link as one staging block (klatt_export.h) through one of kExportSlots page-locked / device buffer
// pairs; nothing waits on the host unless all slots hold exports in flight or a buffer of the batch must grow.  An entry point is
//     batch_entry        the C-ABI shell: begin_call, the "no batch" refusal, no exception leaves
//     (its own argument refusals)
//     export_selection   the chosen utterances: the range refusal and one row per choice
//     export_elements    the extent refusals; zero elements return 0 here, before the output is looked at
//     export_output      the batch's device and the caller's output on it
//     ExportStage        begin() ... the launches ... finish()
// in this order, which is the order of its refusals: those of the arguments come before anything touches the device.

// A table the exports share grows: the exports in flight may read it, so the host waits for them first.
template <typename T>
int grow_table(Batch* b, DeviceBuffer<T>& buf, size_t n)
{
    if (n > buf.cap && settle_track_exports(b, true)) return -1;
    return buf.reserve(std::max<size_t>(n, 1));
}

// The per-request records behind the set call on stream `st`: built by the first export after a set call, waited for by the others.
int timeline_on_stream(Batch* b, hipStream_t st)
{
    if (b->timelineFresh) { HIP_TRY(hipStreamWaitEvent(st, b->timelineReady, 0)); return 0; }
    if (grow_table(b, b->dTimeline, (size_t)b->nFrames)) return -1;
    HIP_TRY(hipStreamWaitEvent(st, b->setDone, 0));
    HIP_TRY(hipStreamWaitEvent(st, b->setCopied, 0));
    const unsigned grid = (unsigned)std::min<long long>((b->nLists + 255) / 256, 4ll * b->cus);
    hipLaunchKernelGGL(klatt_timeline_requests, dim3(std::max(grid, 1u)), dim3(256), 0, st, b->dMeta.ptr, b->dListStart.ptr, b->nLists, b->dTimeline.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->timelineReady, st));
    b->timelineFresh = true;
    return 0;
}

template <class Fn>
long long batch_entry(const char* what, speechPlayer_batch_t batch, Fn fn)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) { set_error("%s: no batch", what); return -1; }
    try {
        return fn(b);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

// The choice of an export: utterances[0 .. nUtterances) (null: every utterance, in order), each an utterance of the batch.  Its
// number, or -1 with the message set.  frameLimit: the export's kernels index the frames by 32 bits.
long long check_selection(Batch* b, const char* what, const long long* utterances, long long nUtterances, bool frameLimit)
{
    const long long n = utterances ? nUtterances : b->nUtt;
    if (n < 0) { set_error("%s: %lld utterances", what, n); return -1; }
    if (frameLimit && b->nFrames >= 0xFFFFFFFFll) { set_error("%s: too many frames", what); return -1; }
    for (long long i = 0; utterances && i < n; ++i)
        if (utterances[i] < 0 || utterances[i] >= b->nUtt) { set_error("%s: utterances[%lld] = %lld is not an utterance of the batch (%lld)", what, i, utterances[i], b->nUtt); return -1; }
    return n;
}

// The rows of an export, one per chosen utterance in the order chosen: perRow(i, u, before) makes row i from utterance u and answers
// its count of entries (negative: it has set the message); `before` is the sum of the counts of rows 0 .. i - 1.
struct ExportSelection {
    long long n = 0, most = 0, total = 0;
    std::vector<long long> counts;
};
// The same over the rows of a caller's signal: rows[0 .. nRows) (null: every row, in order), each a row of the signal
long long check_signal_rows(const char* what, const SignalPlan& sig, const long long* rows, long long nRows)
{
    const long long n = rows ? nRows : sig.nRows;
    if (n < 0) { set_error("%s: %lld rows", what, n); return -1; }
    for (long long i = 0; rows && i < n; ++i)
        if (rows[i] < 0 || rows[i] >= sig.nRows) { set_error("%s: rows[%lld] = %lld is not a row of the signal (%lld)", what, i, rows[i], sig.nRows); return -1; }
    return n;
}
template <class PerRow>
int export_selection(Batch* b, const char* what, const long long* utterances, long long nUtterances, bool frameLimit, ExportSelection& s, PerRow perRow,
                     const SignalPlan* sig = nullptr)
{
    s.n = sig ? check_signal_rows(what, *sig, utterances, nUtterances) : check_selection(b, what, utterances, nUtterances, frameLimit);
    if (s.n < 0) return -1;
    s.counts.resize((size_t)s.n);
    for (long long i = 0; i < s.n; ++i) {
        const long long count = perRow(i, utterances ? utterances[i] : i, s.total);
        if (count < 0) return -1;
        s.counts[(size_t)i] = count;
        s.most = std::max(s.most, count);
        s.total += count;
    }
    return 0;
}

// The elements of the export (klatt_export.h: export_extent), or -1 with the message set.
long long export_elements(const char* what, const ExportNouns& nouns, const ExportSelection& s, long long rowStride, long long perEntry,
                          long long capacity = kNoCapacity)
{
    std::string why;
    const long long elements = export_extent(nouns, s.most, s.total, s.n, rowStride, perEntry, capacity, why);
    if (elements < 0) set_error("%s: %s", what, why.c_str());
    return elements;
}

// One export's passage through a slot.  begin(): the slot (the host waits only if its last export is still in flight), the caller's
// tables (`grow`) -- every allocation first: once a kernel is queued the slot's event must come to stand behind it -- then the
// per-request records, the shared table's previous export, and the block's upload on the stream.  finish(): behind the launches.
// An export of the batch's PCM (ofPcm: the spectrogram) reads the pool instead: it takes one of speechPlayer_batch_exportPcm's slots, which
// the next launch waits for (wait_exports), and stands behind the batch's last launch (pcmReady) in place of the per-request records.
// An export of a caller's signal (ofSignal) reads nothing of the batch: it takes a slot of the exports "as set" -- no launch waits for
// it -- and stands behind nothing; the caller orders whatever produces the signal before it on `st`.  It works on a batch never set.
struct ExportStage {
    Batch* b;
    hipStream_t st;
    const StageBlock& block;
    Batch::SharedTable* table;      // the order the export's shared table keeps (null: it uses none)
    bool ofPcm, ofSignal;
    Batch::ExportSlot* slot = nullptr;
    ExportStage(Batch* b, hipStream_t st, const StageBlock& block, Batch::SharedTable* table = nullptr, bool ofPcm = false, bool ofSignal = false)
        : b(b), st(st), block(block), table(table), ofPcm(ofPcm), ofSignal(ofSignal) {}
    template <class Grow>
    int begin(Grow grow)
    {
        slot = ofPcm ? &b->exportSlot[b->exportNext++ % Batch::kExportSlots] : &b->trackSlot[b->trackNext++ % Batch::kExportSlots];
        if (slot->used) { HIP_TRY(hipEventSynchronize(slot->done)); slot->used = false; }
        if (slot->host.ensure(block.upload_bytes()) || slot->dev.reserve(block.bytes())) return -1;      // (reserved sections at the block's end are device scratch alone)
        if (grow()) return -1;
        if (ofPcm) {
            HIP_TRY(hipEventRecord(b->pcmReady, b->stream));
            HIP_TRY(hipStreamWaitEvent(st, b->pcmReady, 0));
        } else if (!ofSignal && timeline_on_stream(b, st)) return -1;
        if (table && table->wait(st)) return -1;
        block.copy_to(slot->host.ptr);
        if (block.upload_bytes()) HIP_TRY(hipMemcpyAsync(slot->dev.ptr, slot->host.ptr, block.upload_bytes(), hipMemcpyHostToDevice, st));
        return 0;
    }
    int begin() { return begin([] { return 0; }); }
    template <class T> const T* device(int section) const { return block.device<T>(section, slot->dev.ptr); }
    int finish()
    {
        HIP_TRY(hipEventRecord(slot->done, st));
        slot->used = true;
        return table ? table->mark(st) : 0;
    }
};
// (the staging block's sections start on 16-byte boundaries: no kernel takes two of them for one array)
static_assert(sizeof(TimelineRow) % 8 == 0 && sizeof(AlignRow) % 8 == 0 && sizeof(EpochRow) % 8 == 0 && sizeof(SourceList) % 8 == 0 &&
              sizeof(TimelineList) % 8 == 0 && sizeof(StemRow) % 8 == 0 && sizeof(ResponseGroup) % 8 == 0 && sizeof(SpecRow) % 8 == 0 &&
              sizeof(ResRow) % 8 == 0 && sizeof(ConvRow) % 8 == 0 && sizeof(MixRow) % 8 == 0 && sizeof(MixTermDev) % 8 == 0 &&
              sizeof(MixGainJob) % 8 == 0 && sizeof(PowerJob) % 8 == 0, "rows are arrays of 8-byte words");

// How many of the quiet, nasal-free utterances (the head of `order`) the lane-pipelined kernel takes.
// layout 2 forces it; "auto" takes it where it measured faster than the stage-parallel kernel.
long long lanepipe_count(const Batch* b)
{
    if (b->layout == 2) return b->nNoNasal;
    if (b->layout != -1 || b->nNoNasal == 0) return 0;
    // Its workgroups hold 16 utterances against 64, at ~30 ns per sample against 46 for the stage-parallel kernel's
    // slowest stage (MI355X, tools/len_probe.py): it wins while every workgroup of the launch has a CU of its own --
    // 0.75 against 1.2 ms at 4096 vowels -- and loses beyond (8192 vowels: two workgroups per CU).
    const long long groups = (b->nNoNasal + kLpUPG - 1) / kLpUPG + (b->nSlots - b->nNoNasal + kLanes - 1) / kLanes;
    return groups <= b->cus ? b->nNoNasal : 0;
}

// How many of the noisy utterances (the head of the noisy part of `order`) take their coefficients from tracks: those the
// host planned tracks for, under the stage-parallel layouts.
#ifndef KLATT_FLAT_CH
#define KLATT_FLAT_CH 16
#endif
#ifndef KLATT_FLAT_WPS
#define KLATT_FLAT_WPS 2
#endif

// The track planner, the shape table and the fades' end points are klatt_trackplan.h; the host's worker threads klatt_hostpool.h.
// speechPlayer_setGlobalOption("plan_hash_bits"): read once per set call or planning view, on the calling thread (plan_hash_mask),
// and handed to the planner by value -- no planner thread reads it.
std::atomic<unsigned long long> g_planHashMask[2] = {{~0ull}, {~0ull}};
HashMask plan_hash_mask() { return HashMask{g_planHashMask[0].load(std::memory_order_relaxed), g_planHashMask[1].load(std::memory_order_relaxed)}; }

// (Timing-only experiment builds -- wrong PCM, kept as a patch under tools/variants/ since round 5 -- define KLATT_TIMING_ONLY_BUILD: such a
// library refuses to hand PCM out, it only times.  ADVICE r3.)
#ifdef KLATT_TIMING_ONLY_BUILD
constexpr bool kTimingOnlyBuild = true;
#else
constexpr bool kTimingOnlyBuild = false;
#endif
bool refuse_timing_only(const char* what)
{
    if (!kTimingOnlyBuild || getenv("SPEECHPLAYER_ALLOW_TIMING_ONLY_PCM")) return false;
    set_error_code(SPEECHPLAYER_ERR_ARGUMENT);
    set_error("%s: this library was built with a timing-only experiment switch; its PCM is not valid", what);
    return true;
}

long long tracked_count(const Batch* b) { return (b->tracks && b->layout != 0) ? b->nTracked : 0; }
// (setUtterances only forms the direct group under the stage-parallel layouts)
long long direct_count(const Batch* b) { return b->nDirect; }
// The direct stages' residency for a launch of nGroups workgroups (option "direct_lean").  The engine's choice (tools/direct_size_probe.py,
// all-different batches of 8192 .. 65 536 utterances): MODE_FAST takes the lean stages -- two workgroups per CU -- at every size (12.4
// against 12.8 ms at 128 workgroups, 13.4 / 14.5 at 512, 18.1 / 27.3 at 1024); MODE_EXACT once the launch has more than TWO workgroups
// per CU (a launch of up to 512 workgroups lasts as long as its longest utterance takes through one workgroup's pipeline, which is
// shorter with the CU to itself: 26.4 against 27.7 ms at 512 workgroups; 31.7 / 30.0 at 576, 50.6 / 37.7 at 1024) -- and neither when
// the lanes are time-aligned: the lean stages have no steady path of their own (an aligned batch spends most chunks there: cfg2
// without its tracks 13.9 ms against 16.4, MODE_FAST; "distinct" 14.3 / 15.2).
bool direct_lean(const Batch* b, long long nGroups)
{
    if (b->directLean >= 0) return b->directLean != 0;
    if (b->directAligned) return false;
    return b->mode == MODE_FAST ? true : nGroups > 2ll * b->cus;
}

int batch_launch(Batch* b)
{
    KernelArgs a = base_args(b->sampleRate);
    a.frames = b->dFrames.ptr; a.meta = b->dMeta.ptr; a.utt = b->dUtt.ptr;
    a.pcm = b->dPcm.ptr; a.result = b->dResult.ptr; a.state = nullptr; a.control = nullptr;
    if (wait_exports(b)) return -1;      // (the pool is overwritten: exports queued on other streams read it first)
    b->resultsFresh = false;
    b->floatFresh = false;
    b->launched = true;
#ifdef KLATT_STAMPS
    if (b->dDebug.reserve((size_t)(b->nSlots / kLpUPG + 2) * 32 * 2)) return -1;
    HIP_TRY(hipMemsetAsync(b->dDebug.ptr, 0, b->dDebug.cap * 8, b->stream));
    a.debug = b->dDebug.ptr;
#endif
    // up to four groups, each with its own kernel, side by side on their own streams:
    //   order[0, nLp)              quiet, nasal-free -> lane-pipelined kernel (klatt_lanepipe.h), when the plan takes it
    //   order[nLp, nNoNasal)       quiet, nasal-free -> stage-parallel kernel without the nasal pair (NASAL = false)
    //   order[nNoNasal, nQuiet)    quiet             -> stage-parallel (or lane) kernel, NOISE = false
    //   order[nQuiet, nSlots)      noisy             -> stage-parallel (or lane) kernel, NOISE = true
    //   order[nQuiet, nQuiet + nTr)  noisy, tracked  -> klatt_tracks, then the stage-parallel kernel with flat stages (FLAT = true)
    const long long nLp = lanepipe_count(b);
    const bool laneKernel = b->layout == 0;
    const long long nTr = tracked_count(b);
    const long long nDir = direct_count(b);
    // the noisy utterances that run on the stages with the frame state machine: the tail of `order`, and the tracked group's slots
    // when the tracks were planned but have been switched off since (options are read by setUtterances; "tracks" also here)
    const long long nNoisyHead = b->nTracked - nTr;
    const long long nNoisy = b->nSlots - b->nQuiet - b->nTracked - nDir;
    const long long nNn = laneKernel ? 0 : b->nNoNasal - nLp;
    const long long nQ = b->nQuiet - nLp - nNn;
    const int parts = (nLp > 0) + (nNn > 0) + (nQ > 0) + (nNoisy > 0) + (nNoisyHead > 0) + (nTr > 0) + (nDir > 0);
    const bool fork = parts > 1;
    if (fork) HIP_TRY(hipEventRecord(b->forkEvent, b->stream));
    int sideUsed = 0, seen = 0;
    // The last group launched runs on the main stream, the others beside it.  The QUIET groups are launched AFTER the noisy ones (option
    // "quiet_last", default 1): the noisy workgroups are few, long jobs (configs[2]: 896 workgroups of 8 273 .. 41 238 steps on 512
    // slots, whose best schedule ends with half the chip idle), the quiet ones cost a third per step -- dispatched behind the noisy
    // grid they take the slots it leaves free instead of delaying its longest jobs: configs[2] 8.44 -> 8.39 ms, MODE_FAST 7.88 -> 7.68,
    // configs[4]'s share 62.6 -> 62.2 (tools/quiet_priority_probe.py; low-PRIORITY streams for them were measured too and lost: 8.9 ms).
    auto next_stream = [&](bool = false) -> hipStream_t {
        if (!fork || ++seen == parts) return b->stream;
        hipStream_t st = b->side[sideUsed++];
        (void)hipStreamWaitEvent(st, b->forkEvent, 0);
        return st;
    };
    const GroupPlan plq = plan_group(b->layout, false, b->nSlots, nNoisy, b->cus);
    auto launch_quiet = [&]() -> int {
    if (nLp > 0) {
        hipStream_t st = next_stream(true);
        a.order = b->dOrder.ptr; a.nSlots = nLp;
        const long long g = (nLp + kLpUPG - 1) / kLpUPG;
        if (g <= b->cus ? launch_lanepipe<KLATT_LP_CH, 1>(a, b->mode, g, st) : launch_lanepipe<16, 2>(a, b->mode, g, st)) return -1;
    }
    if (nNn > 0) {
        hipStream_t st = next_stream(true);
        a.order = b->dOrder.ptr + nLp; a.nSlots = nNn;
        const long long g = (nNn + kLanes - 1) / kLanes;
        if (plq.chunk == 32 ? launch_systolic<false, 32, 1, false>(a, b->mode, g, st) : launch_systolic<false, 16, 2, false>(a, b->mode, g, st)) return -1;
    }
    if (nQ > 0) {
        hipStream_t st = next_stream(true);
        a.order = b->dOrder.ptr + nLp + nNn; a.nSlots = nQ;
        const long long g = (nQ + kLanes - 1) / kLanes;
        if (plq.systolic ? (plq.chunk == 32 ? launch_systolic<false, 32>(a, b->mode, g, st) : launch_systolic<false, 16>(a, b->mode, g, st))
                         : launch<false, false>(a, b->mode, g, st)) return -1;
    }
        return 0;
    };
    // (behind FLAT or direct stages only: the stages with the frame state machine fill the CU's LDS two workgroups at a time, and quiet
    // workgroups queued behind them wait for the launch's tail -- the benchmarked batch without its tracks 13.8 -> 14.7 ms)
    const bool quietLast = b->quietLast && (nTr > 0 || nDir > 0) && nNoisy == 0 && nNoisyHead == 0;
    if (!quietLast && launch_quiet()) return -1;
    if (nTr > 0) {
        hipStream_t st = next_stream();
        TrackArgs t;
        t.jobs = b->dJobs.ptr; t.nJobs = b->nJobs; t.shapes = b->dShapes.ptr; t.track = b->dTrack.ptr;
        t.negPiOverSr = a.negPiOverSr; t.twoPiOverSr = a.twoPiOverSr;
        const long long tg = b->nJobs;     // one workgroup per track
        if (tg > 0x7FFFFFFF) { set_error("too many tracks: %lld", b->nJobs); return -1; }
        // (eight words, not seven: a fill of 28 bytes goes out as two kernels, one of 32 as one)
        if (b->dDeadWaves.reserve(8)) return -1;
        static_assert(3 + kDead2Counts <= 8, "the counters' block");
        HIP_TRY(hipMemsetAsync(b->dDeadWaves.ptr, 0, 8 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(klatt_tracks, dim3((unsigned)tg), dim3(kLanes * kTrackWaves), 0, st, t);
        HIP_TRY(hipGetLastError());
        a.order = b->dOrder.ptr + b->nQuiet; a.nSlots = nTr;
        a.flatRef = b->dFlatRef.ptr; a.sourceRef = b->dSourceRef.ptr; a.track = b->dTrack.ptr;
        a.trackBytes = (uint32_t)std::min<unsigned long long>(((unsigned long long)b->trackEntries + kTrackPad) * sizeof(double2), 0xFFFFFFFFull);
        // the terms a wavefront may drop (read by every launch, like "tracks"), and how many did (counters zeroed ahead of klatt_tracks)
        a.deadWaves = b->dDeadWaves.ptr; a.deadTerms = b->deadTerms ? kUttPresent : 0u;
        a.present2 = b->dPresent2.ptr; a.deadTerms2 = (b->deadTerms && b->dPresent2.ptr) ? kUtt2Present : 0u;
        const GroupPlan pl = plan_group(b->layout, true, b->nSlots, nTr + nNoisy, b->cus);
        const long long g = (nTr + kLanes - 1) / kLanes;
        // flat stages keep nothing but the pipes and the PCM tile in LDS: 16-sample hand-overs fit two workgroups per CU (70 KB each)
        if (pl.chunk == 8 ? launch_systolic<true, KLATT_FLAT_CH, KLATT_FLAT_WPS, true, false, true>(a, b->mode, g, st)
                          : launch_systolic<true, 16, 1, true, false, true>(a, b->mode, g, st)) return -1;
        a.flatRef = nullptr; a.sourceRef = nullptr; a.track = nullptr; a.deadWaves = nullptr; a.deadTerms = 0u; a.present2 = nullptr; a.deadTerms2 = 0u;
    }
    if (nDir > 0) {
        hipStream_t st = next_stream();
        SeedArgs sa;
        sa.jobs = b->dDirectJobs.ptr; sa.nJobs = (uint32_t)b->nDirectFrames; sa.frames = b->dFrames.ptr; sa.meta = b->dMeta.ptr;
        sa.hdr = b->dDirectHdr.ptr; sa.rec = b->dDirectRec.ptr; sa.negPiOverSr = a.negPiOverSr; sa.twoPiOverSr = a.twoPiOverSr;
        const dim3 sg((unsigned)((b->nDirectFrames + 255) / 256), (unsigned)kDirectStages);
        constexpr int kSeedLds = 14 * 257 * (int)sizeof(double2);      // the largest record (14 entries) of 256 frames, pitch 257 (seed_stage)
        if (b->mode == MODE_FAST) hipLaunchKernelGGL(klatt_seeds<MODE_FAST>, sg, dim3(256), kSeedLds, st, sa);
        else hipLaunchKernelGGL(klatt_seeds<MODE_EXACT>, sg, dim3(256), kSeedLds, st, sa);
        HIP_TRY(hipGetLastError());
        a.order = b->dOrder.ptr + b->nQuiet + b->nTracked; a.nSlots = nDir;
        a.directHdr = b->dDirectHdr.ptr; a.directRec = b->dDirectRec.ptr; a.directFirst = b->dDirectFirst.ptr; a.nDirect = (uint32_t)b->nDirectFrames;
        a.sourceRef = b->dSourceRef.ptr;
        const long long g = (nDir + kLanes - 1) / kLanes;
        if (launch_direct(a, b->mode, direct_lean(b, g), g, st)) return -1;
        a.directHdr = nullptr; a.directRec = nullptr; a.directFirst = nullptr; a.nDirect = 0; a.sourceRef = nullptr;
    }
    for (int half = 0; half < 2; ++half) {
        const long long n = half ? nNoisy : nNoisyHead;
        if (n <= 0) continue;
        hipStream_t st = next_stream();
        a.order = b->dOrder.ptr + b->nQuiet + (half ? b->nTracked + nDir : 0); a.nSlots = n;
        const GroupPlan pl = plan_group(b->layout, true, b->nSlots, nTr + nNoisy + nNoisyHead, b->cus);
        const long long g = (n + kLanes - 1) / kLanes;
        if (pl.systolic ? (pl.chunk == 8 ? launch_systolic<true, KLATT_NOISY_CH, 2>(a, b->mode, g, st) : launch_systolic<true, 16>(a, b->mode, g, st))
                        : launch<false, true>(a, b->mode, g, st)) return -1;
    }
    if (quietLast && launch_quiet()) return -1;
    for (int i = 0; i < sideUsed; ++i) {
        HIP_TRY(hipEventRecord(b->join[i], b->side[i]));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->join[i], 0));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Streams behind the reference's five entry points
// ------------------------------------------------------------------------------------------
// What a live handle owns lives in ONE arena per device, indexed by the handle's slot: its saved synthesiser state
// (kStateDoubles doubles) and a ring of kRing frames.  A queued frame is written once, into a pinned log
// (speechPlayer_queueFrame), the log travels in one copy and a scatter kernel drops its entries into the rings; a pull
// uploads one control block (what to do for each handle of the call) and whatever part of the log has not travelled yet.
// Nothing a handle queued is staged again on a later pull (reference contract: src/frame.cpp:90-115 queue, :54-75 dequeue).
// The host's bookkeeping of all this -- a handle's ring and host queue, the log's indices, the options, the plan of a pull -- is
// klatt_live.h, which has no HIP in it and a native test of its own; here are the memory, the copies and the launches.
constexpr size_t kLogEntries = 40960;            // 16 MB of pinned log
constexpr size_t kLogEager = 2560;               // queueFrame sends the log on its way once 1 MB waits (if no pull is running)

struct LogEntry {            // 400 B
    double p[kNumParams];
    FrameMeta meta;
    uint32_t target;         // slot * kRing + ring position, or kNoTarget (purged / handle closed before the entry travelled)
    uint32_t pad;
};
static_assert(sizeof(LogEntry) == 400, "LogEntry layout");

__global__ void __launch_bounds__(256) live_scatter(const LogEntry* __restrict__ log, uint32_t n, double* __restrict__ ringFrames,
                                                    FrameMeta* __restrict__ ringMeta)
{
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6), j = threadIdx.x & 63u;     // one wavefront per entry
    if (e >= n) return;
    const uint32_t at = log[e].target;
    if (at == kNoTarget) return;
    if (j < (uint32_t)kNumParams) ringFrames[(size_t)at * kNumParams + j] = log[e].p[j];
    else if (j == (uint32_t)kNumParams) ringMeta[at] = log[e].meta;
}

// speechPlayer_queueFramesManyDevice: a frame in the caller's device memory into the ring position the host assigned it -- the log's
// entry without its 376 bytes of values, which the kernel reads from the caller's row instead (row -1: a NULL frame, zeros as
// log_append writes them; such a row is never read).
struct LivePlace {           // 32 B
    FrameMeta meta;
    long long row;           // the frame's row of the caller's array, or -1
    uint32_t target;         // slot * kRing + ring position
    uint32_t pad;
};
static_assert(sizeof(LivePlace) == 32, "LivePlace layout");

__global__ void __launch_bounds__(256) live_place(const double* __restrict__ frames, const LivePlace* __restrict__ place, long long n,
                                                  double* __restrict__ ringFrames, FrameMeta* __restrict__ ringMeta)
{
    const uint32_t j = threadIdx.x & 63u;
    const long long step = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += step) {     // one wavefront per frame
        const LivePlace p = place[e];
        if (j < (uint32_t)kNumParams) ringFrames[(size_t)p.target * kNumParams + j] = p.row < 0 ? 0.0 : frames[p.row * kNumParams + j];
        else if (j == (uint32_t)kNumParams) ringMeta[p.target] = p.meta;
    }
}

struct Stream {
    int sampleRate = 0;
    int device = 0;
    int mode = MODE_EXACT;
    uint32_t seed = 0;
    uintptr_t id = 0;
    std::mutex mu;                       // per call, not per sample (reference locks per sample: src/frame.cpp:122)
    struct LiveContext* context = nullptr;   // the device's live-handle context
    uint32_t slot = 0;                   // its place in the device's arena
    FrameQueue q;                        // its ring, and what waits on the host behind it
    LogMine logged;                      // its entries in the part of the log that has not travelled
    int lastIndex = -1;
};

std::mutex g_tableMutex;
std::vector<Stream*> g_streams;   // handle = index + 1

Stream* lookup_locked(speechPlayer_handle_t h)
{
    uintptr_t id = reinterpret_cast<uintptr_t>(h);
    // a prototype-less 32-bit ctypes call hands the id back sign-/zero-extended; ids are small
    id &= 0xFFFFFFFFu;
    if (id == 0 || id > g_streams.size()) return nullptr;
    return g_streams[id - 1];
}
Stream* lookup(speechPlayer_handle_t h)
{
    std::lock_guard<std::mutex> g(g_tableMutex);
    return lookup_locked(h);
}

template <typename T>
struct PinnedBuffer {
    T* ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        n = std::max(n, cap * 2);          // contents are not kept
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr; cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T), hipHostMallocDefault));
        cap = n;
        return 0;
    }
};

// The live handles of one device: arena, log, launch buffers.  Lock order: Stream::mu, then LiveContext::mu, then logMu.
// `mu` serialises everything that enqueues on `stream` or moves the arena; `logMu` only guards the log's indices, so that
// queueFrame on one handle does not wait for a pull of other handles.
struct LiveContext {
    std::mutex mu;
    hipStream_t stream = nullptr;
    // arena
    uint32_t slots = 0, nextSlot = 0;
    std::vector<uint32_t> freeSlots;
    DeviceBuffer<double> dState;         // [slots][kStateDoubles]
    DeviceBuffer<double> dRingFrames;    // [slots][kRing][kNumParams]
    DeviceBuffer<FrameMeta> dRingMeta;   // [slots][kRing]
    // log
    std::mutex logMu;
    PinnedBuffer<LogEntry> hLog;
    DeviceBuffer<LogEntry> dLog;
    LogIndex<LogEntry> log;              // over hLog
    // one pull
    PinnedBuffer<unsigned char> hCtl;    // UttDesc[n] | state pointer[n] | control[n], one copy
    DeviceBuffer<unsigned char> dCtl;
    PinnedBuffer<UttResult> hResult;
    DeviceBuffer<UttResult> dResult;
    DeviceBuffer<uint32_t> dOrder;       // 0, 1, 2, ...: written once
    size_t orderFilled = 0;
    DeviceBuffer<int16_t> dPcm, dPcmJoin;
    std::vector<uint32_t> done;
    PinnedPair bounce;
    hipEvent_t kernelStart = nullptr, kernelStop = nullptr;
    float lastKernelMs = 0.0f;           // the last call's kernel time (speechPlayer_lastLiveKernelMs)
    int lastLaunches = 0;
    int cus = 256;                       // the device's CUs (pcm_export's grid)
    // speechPlayer_queueFramesManyDevice: ring frames placed by live_place from the caller's memory, the rows of frames that go to the
    // host queues gathered (klatt_gather_frames) and downloaded; `stream` first waits for inputReady, recorded on the caller's stream
    hipEvent_t inputReady = nullptr;
    PinnedBuffer<LivePlace> hPlace;
    DeviceBuffer<LivePlace> dPlace;
    PinnedBuffer<long long> hGatherIdx;
    DeviceBuffer<long long> dGatherIdx;
    PinnedBuffer<double> hGatherRows;
    DeviceBuffer<double> dGatherRows;
    // speechPlayer_synthesizeManyExport: pcm_export on the caller's stream behind pullDone, its rows staged through one of kExportSlots
    // page-locked / device buffer pairs; the next pull waits for the exports on the device before it overwrites dPcm / dPcmJoin, the
    // host waits for them before either is freed (live_wait_exports)
    hipEvent_t pullDone = nullptr;
    struct ExportSlot { PinnedBlock host; DeviceBuffer<unsigned char> dev; hipEvent_t done = nullptr; bool used = false, pending = false; };
    static constexpr int kExportSlots = 16;
    ExportSlot exportSlot[kExportSlots];
    unsigned exportNext = 0;
};
std::mutex g_liveMutex;
std::vector<LiveContext*> g_live;   // per device
LiveOptions g_liveOptions;          // speechPlayer_setGlobalOption's "live_*"; a pull, initialize and terminate read one snapshot() each
static_assert(MODE_EXACT == 0 && MODE_FAST == 1, "live_mode's values (klatt_live.h)");

// c->mu held.  No handle lives on this device: give its arena (state blocks, rings) and the pull buffers back.  The next
// speechPlayer_initialize starts a new arena of 64 slots.
// c->mu held.  Exports of earlier pulls (speechPlayer_synthesizeManyExport) may still read dPcm / dPcmJoin on their callers' streams:
// before the buffers are overwritten `stream` waits for them on the device; before they are freed (freeing) the host waits.
int live_wait_exports(LiveContext* c, bool freeing)
{
    for (auto& e : c->exportSlot) {
        if (!e.used) continue;
        if (freeing) { HIP_TRY(hipEventSynchronize(e.done)); e.used = e.pending = false; }
        else if (e.pending) { HIP_TRY(hipStreamWaitEvent(c->stream, e.done, 0)); e.pending = false; }
    }
    return 0;
}

void arena_trim(LiveContext* c)
{
    if (c->slots == 0 || c->freeSlots.size() != (size_t)c->nextSlot) return;
    (void)hipStreamSynchronize(c->stream);
    (void)live_wait_exports(c, true);
    c->dState.release(); c->dRingFrames.release(); c->dRingMeta.release();
    c->dPcm.release(); c->dPcmJoin.release(); c->dCtl.release(); c->dResult.release(); c->dOrder.release();
    c->dPlace.release(); c->dGatherIdx.release(); c->dGatherRows.release();
    for (auto& e : c->exportSlot) e.dev.release();
    c->orderFilled = 0;
    c->slots = 0; c->nextSlot = 0;
    c->freeSlots.clear();
}

LiveContext* live_context(int device)
{
    std::lock_guard<std::mutex> g(g_liveMutex);
    if ((int)g_live.size() <= device) g_live.resize(device + 1, nullptr);
    if (!g_live[device]) {
        LiveContext* c = new LiveContext;
        bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreate(&c->kernelStart) == hipSuccess && hipEventCreate(&c->kernelStop) == hipSuccess &&
                  hipEventCreateWithFlags(&c->inputReady, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&c->pullDone, hipEventDisableTiming) == hipSuccess &&
                  !c->hLog.reserve(kLogEntries) && !c->dLog.reserve(kLogEntries);
        for (auto& e : c->exportSlot) ok = ok && hipEventCreateWithFlags(&e.done, hipEventDisableTiming) == hipSuccess;
        hipDeviceProp_t prop;
        if (ok && hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->cus = prop.multiProcessorCount;
        if (!ok) {
            set_error("cannot create the live-handle context of device %d", device);
            delete c;
            return nullptr;
        }
        c->log.entries = c->hLog.ptr; c->log.cap = c->hLog.cap;
        g_live[device] = c;
    }
    return g_live[device];
}

// c->mu held.  Room for `want` slots: the arena doubles, what the handles saved moves along (device to device).
int arena_reserve(LiveContext* c, uint32_t want)
{
    if (want <= c->slots) return 0;
    uint32_t cap = std::max<uint32_t>(64, c->slots);
    while (cap < want) cap *= 2;
    DeviceBuffer<double> st, fr;
    DeviceBuffer<FrameMeta> me;
    if (st.reserve((size_t)cap * kStateDoubles) || fr.reserve((size_t)cap * kRing * kNumParams) || me.reserve((size_t)cap * kRing)) {
        st.release(); fr.release(); me.release();
        return -1;
    }
    if (c->slots) {
        HIP_TRY(hipMemcpyAsync(st.ptr, c->dState.ptr, (size_t)c->slots * kStateDoubles * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(fr.ptr, c->dRingFrames.ptr, (size_t)c->slots * kRing * kNumParams * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(me.ptr, c->dRingMeta.ptr, (size_t)c->slots * kRing * sizeof(FrameMeta), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->dState.release(); c->dRingFrames.release(); c->dRingMeta.release();
    c->dState = st; c->dRingFrames = fr; c->dRingMeta = me;
    c->slots = cap;
    return 0;
}

int stream_init_device(Stream* s)
{
    LiveContext* c = live_context(s->device);
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(s->device));
    uint32_t slot;
    if (!c->freeSlots.empty()) { slot = c->freeSlots.back(); c->freeSlots.pop_back(); }
    else {
        if (arena_reserve(c, c->nextSlot + 1)) return -1;
        slot = c->nextSlot++;
    }
    s->slot = slot; s->context = c;
    HIP_TRY(hipMemsetAsync(c->dState.ptr + (size_t)slot * kStateDoubles, 0, kStateDoubles * sizeof(double), c->stream));   // ordered before the handle's first pull
    return 0;
}

// c->mu and c->logMu held.  What waits in the log goes on its way: one copy, one scatter launch; not waited for.
int log_send(LiveContext* c)
{
    const size_t n = c->log.waiting(), from = c->log.sent;
    if (n == 0) return 0;
    HIP_TRY(hipMemcpyAsync(c->dLog.ptr + from, c->hLog.ptr + from, n * sizeof(LogEntry), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(live_scatter, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, c->dLog.ptr + from, (uint32_t)n,
                       c->dRingFrames.ptr, c->dRingMeta.ptr);
    HIP_TRY(hipGetLastError());
    c->log.mark_sent();
    return 0;
}

// s->mu held.  One frame into the handle's ring at the position claimed for it (FrameQueue::claim), by way of the log.
int log_append(LiveContext* c, Stream* s, const double* p, const FrameMeta& meta, uint32_t pos, bool holdsContext)
{
    std::unique_lock<std::mutex> lg(c->logMu);
    LogEntry* e = c->log.append(s->logged);
    if (!e) {                            // full: send it, wait until it has arrived, start over (lock order: mu before logMu)
        std::unique_lock<std::mutex> g(c->mu, std::defer_lock);
        if (!holdsContext) { lg.unlock(); g.lock(); lg.lock(); }
        e = c->log.append(s->logged);
        if (!e) {
            HIP_TRY(hipSetDevice(s->device));
            if (log_send(c)) return -1;
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->log.arrived();
            e = c->log.append(s->logged);
        }
    }
    if (p) memcpy(e->p, p, sizeof e->p); else memset(e->p, 0, sizeof e->p);
    e->meta = meta;
    e->target = s->slot * kRing + pos;
    e->pad = 0;
    return 0;
}

// s->mu held.  Forget what the handle has in the ring and in the log (close; the device half of a purge).
void ring_drop(LiveContext* c, Stream* s)
{
    std::lock_guard<std::mutex> lg(c->logMu);
    c->log.untarget(s->logged);
    s->q.drop();
}

// s->mu held.  A purge request: FrameQueue::purge, and the handle's waiting log entries go nowhere.
void stream_purge(LiveContext* c, Stream* s)
{
    { std::lock_guard<std::mutex> lg(c->logMu); c->log.untarget(s->logged); }
    s->q.purge();
}

// speechPlayer_synthesizeManyExport: where a pull's rows go (caller-owned device memory the entry point has checked).
struct LiveExport { void* out; int format; long long rowStride; hipStream_t stream; };

// c->mu held, the pull just done (it is host-synchronous).  Row i of the pull -- produced[i] samples at pcm + i * padded: the pull
// buffer, or the joined rows of a pull in pieces -- into the caller's row i on the caller's stream (pcm_export), behind pullDone; the
// rows' descriptors are staged through one of kExportSlots page-locked / device buffer pairs, as speechPlayer_batch_exportPcm stages them.
int live_export(LiveContext* c, const int16_t* pcm, size_t padded, const int* produced, int n, const LiveExport& x)
{
    LiveContext::ExportSlot& slot = c->exportSlot[c->exportNext++ % LiveContext::kExportSlots];
    if (slot.used) { HIP_TRY(hipEventSynchronize(slot.done)); slot.used = slot.pending = false; }
    const size_t bytes = (size_t)n * sizeof(ExportRow);
    if (slot.host.ensure(bytes) || slot.dev.reserve(bytes)) return -1;
    ExportRow* rows = static_cast<ExportRow*>(slot.host.ptr);
    for (int i = 0; i < n; ++i) rows[i] = ExportRow{(long long)i * (long long)padded, (long long)produced[i]};
    HIP_TRY(hipEventRecord(c->pullDone, c->stream));
    HIP_TRY(hipStreamWaitEvent(x.stream, c->pullDone, 0));
    HIP_TRY(hipMemcpyAsync(slot.dev.ptr, slot.host.ptr, bytes, hipMemcpyHostToDevice, x.stream));
    const long long elements = (long long)n * x.rowStride, n8 = (elements + 7) / 8;
    const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 8ll * c->cus);
    const int vec = reinterpret_cast<uintptr_t>(x.out) % 16 == 0;
    const ExportRow* dRows = reinterpret_cast<const ExportRow*>(slot.dev.ptr);
    const long long* none = nullptr;       // (rows of rowStride elements: no packed-row index)
    if (x.format) hipLaunchKernelGGL(pcm_export<true>, dim3(grid), dim3(256), 0, x.stream, pcm, x.out, dRows, none, none, (long long)n, x.rowStride, elements, vec);
    else hipLaunchKernelGGL(pcm_export<false>, dim3(grid), dim3(256), 0, x.stream, pcm, x.out, dRows, none, none, (long long)n, x.rowStride, elements, vec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(slot.done, x.stream));
    slot.used = slot.pending = true;
    return 0;
}

// One pull of n live handles (streams_synthesize): what its steps share.  c->mu and every handle's mutex are held throughout.
struct Pull {
    LiveContext* c;
    Stream* const* ss;
    int n;
    int mode;
    size_t padded;           // samples from a handle's PCM row to the next
    PullPlan plan;
    CtlBlock ctl;
};

// Room for the pull's control block, its results and its PCM; the order 0, 1, 2, ... long enough.
int pull_reserve(const Pull& p)
{
    LiveContext* c = p.c;
    const size_t nCtl = p.ctl.nCtl;
    if (c->hCtl.reserve(p.ctl.bytes()) || c->dCtl.reserve(c->hCtl.cap) || c->hResult.reserve(nCtl) || c->dResult.reserve(c->hResult.cap) ||
        c->dPcm.reserve(p.padded * p.n))
        return -1;
    if (c->orderFilled < nCtl) {
        const size_t m = std::max<size_t>(nCtl, 1024);
        std::vector<uint32_t> iota(m);
        std::iota(iota.begin(), iota.end(), 0u);
        if (c->dOrder.reserve(m)) return -1;
        HIP_TRY(hipMemcpy(c->dOrder.ptr, iota.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->orderFilled = m;
    }
    return 0;
}

// The rings take what waited on the host, by way of the log.  *piece: how far of `want` samples this launch may go without meeting a
// frame that is not in a ring (FrameQueue::reach).
int pull_refill(const Pull& p, unsigned int want, unsigned int* piece)
{
    *piece = want;
    for (int i = 0; i < p.n; ++i) {
        Stream* s = p.ss[i];
        if (s->q.refill([&](const PendingFrame& f, uint32_t pos) { return log_append(p.c, s, (f.meta.flags & FRAME_NULL) ? nullptr : f.p, f.meta, pos, true); }))
            return -1;
        *piece = s->q.reach(*piece);
    }
    return 0;
}

// The control block of a launch of `piece` samples, in page-locked memory.
void pull_fill(const Pull& p, unsigned int piece)
{
    fill_ctl(p.ctl.at(p.c->hCtl.ptr), p.plan, p.n, [&](int i) {
        const Stream* s = p.ss[i];
        CtlEntry e;
        e.utt.frameStart = (long long)s->slot * kRing + s->q.ringHead;
        e.utt.outStart = (long long)(i * p.padded);
        e.utt.nFrames = s->q.ringCount;
        e.utt.seed = s->seed; e.utt.flags = UTT_NEEDS_NOISE;
        e.utt.length = piece;            // the stage-parallel kernel runs exactly `piece` steps (klatt_systolic.h, STREAM)
        e.state = p.c->dState.ptr + (size_t)s->slot * kStateDoubles;
        e.control = s->q.purgePending ? 1u : 0u;
        return e;
    });
}

int pull_launch(const Pull& p, const KernelArgs& a)
{
    hipStream_t st = p.c->stream;
    switch (p.plan.launch) {
    case LiveLaunch::Lane: return launch<true, true>(a, p.mode, p.plan.groups, st);
    case LiveLaunch::Lone: return launch_systolic<true, 16, 1, true, true, false, true>(a, p.mode, p.plan.groups, st);
    case LiveLaunch::StreamOnePerCu: return launch_systolic<true, 16, 1, true, true>(a, p.mode, p.plan.groups, st);
    case LiveLaunch::StreamTwoPerCu: return launch_systolic<true, KLATT_NOISY_CH, 2, true, true>(a, p.mode, p.plan.groups, st);
    }
    return -1;
}

// What the kernel reports, fetched and waited for, into the handles' queues and into done[].
int pull_apply(const Pull& p, unsigned int piece)
{
    LiveContext* c = p.c;
    for (int i = 0; i < p.n; ++i) {
        Stream* s = p.ss[i];
        const UttResult& r = c->hResult.ptr[(size_t)i * p.plan.rep];
        if (r.produced > piece || r.framesTaken > s->q.ringCount) { set_error("kernel produced %u > %u (took %u frames of %u)", r.produced, piece, r.framesTaken, s->q.ringCount); return -1; }
        s->q.took(r.framesTaken);
        s->lastIndex = r.lastIndex;
        c->done[i] += r.produced;
    }
    return 0;
}

// Rows 0 .. rows-1 of the pull (done[i] samples at pcm + i * padded) into their callers' buffers: whole rows in pieces of about 16 MB
// through two pinned buffers; piece k + 1 is in flight while the rows of piece k are handed to their callers.
int pull_hand_out(LiveContext* c, const int16_t* pcm, size_t padded, size_t rows, sample* const* outs)
{
    const size_t rowsPerPiece = std::max<size_t>(1, (8u << 20) / padded);
    if (c->bounce.ensure(rowsPerPiece * padded * sizeof(int16_t))) return -1;
    const size_t nPieces = (rows + rowsPerPiece - 1) / rowsPerPiece;
    auto issue = [&](size_t k) -> int {
        const size_t r0 = k * rowsPerPiece, r1 = std::min(rows, r0 + rowsPerPiece);
        HIP_TRY(hipMemcpyAsync(c->bounce.buf[k & 1], pcm + r0 * padded, (r1 - r0) * padded * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->bounce.ev[k & 1], c->stream));
        return 0;
    };
    if (issue(0)) return -1;
    for (size_t k = 0; k < nPieces; ++k) {
        if (k + 1 < nPieces && issue(k + 1)) return -1;
        HIP_TRY(hipEventSynchronize(c->bounce.ev[k & 1]));
        const size_t r0 = k * rowsPerPiece, r1 = std::min(rows, r0 + rowsPerPiece);
        const int16_t* src = static_cast<const int16_t*>(c->bounce.buf[k & 1]);
        auto rows_out = [&](size_t b0, size_t b1) {
            for (size_t i = b0; i < b1; ++i)
                if (c->done[i]) memcpy(outs[i], src + (i - r0) * padded, (size_t)c->done[i] * sizeof(int16_t));
        };
        // a piece of several megabytes is handed out in four shares side by side (the host's worker pool): one thread's memcpy (about 20 GB/s) is slower than the copy over PCIe
        constexpr unsigned kHands = 4;
        const size_t share = (r1 - r0 + kHands - 1) / kHands;
        if ((r1 - r0) * padded * sizeof(int16_t) >= (4u << 20))
            run_parts(kHands, [&](unsigned t) { const size_t b0 = std::min(r1, r0 + t * share); rows_out(b0, std::min(r1, b0 + share)); });
        else rows_out(r0, r1);
    }
    return 0;
}

// Advance n live streams by up to `count` samples each (one stream per wavefront lane; one launch, unless some handle has
// more frames queued than its ring holds AND the ring's frames end before `count` samples: then the call proceeds in pieces,
// refilling the rings in between -- a pull is the same as several shorter pulls, reference src/speechPlayer.cpp:39-42).
// The callers hold every stream's mutex.  produced[i] receives speechPlayer_synthesize's return value.
// outs == nullptr: the PCM stays on the device (row i at devicePcm + i * stride), for consumers on the GPU.
// The live options are read once, on entry (klatt_live.h: one snapshot, one plan); what is set meanwhile is the next pull's.
#ifdef KLATT_STAMPS
unsigned long long g_streamStamps[32];
extern "C" __attribute__((visibility("default"))) void speechPlayer_debugStreamStamps(unsigned long long* out) { for (int k = 0; k < 32; ++k) { out[k] = g_streamStamps[k]; g_streamStamps[k] = 0; } }
#endif
// exportTo: the rows also go into caller-owned device memory (live_export).
int streams_synthesize(Stream* const* ss, int n, unsigned int count, sample* const* outs, int* produced,
                       const int16_t** devicePcm = nullptr, long long* deviceStride = nullptr, const LiveExport* exportTo = nullptr)
{
    for (int i = 0; i < n; ++i) produced[i] = 0;
    if (count == 0 || n <= 0) return 0;
    static const bool trace = getenv("SPEECHPLAYER_LIVE_TRACE") != nullptr;     // host-side breakdown of a call on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    const LiveSettings options = g_liveOptions.snapshot();
    const int device = ss[0]->device, rate = ss[0]->sampleRate, mode = ss[0]->mode;
    for (int i = 1; i < n; ++i)
        if (ss[i]->device != device || ss[i]->sampleRate != rate || ss[i]->mode != mode) {
            set_error("streams advanced together must share device, sample rate and mode");
            return -1;
        }
    LiveContext* c = live_context(device);
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(device));
    const size_t padded = ((size_t)count + kTile - 1) / kTile * kTile;
    if (live_wait_exports(c, padded * n > c->dPcm.cap)) return -1;
    const PullPlan plan = pull_plan(n, options, c->cus);
    const Pull p{c, ss, n, mode, padded, plan, CtlBlock{(size_t)plan.nCtl}};
    if (pull_reserve(p)) return -1;

    KernelArgs a = base_args(rate);
    const CtlBlock::View dCtl = p.ctl.at(c->dCtl.ptr);
    a.frames = c->dRingFrames.ptr; a.meta = c->dRingMeta.ptr; a.ringMask = kRing - 1;
    a.utt = dCtl.utt; a.statePtrs = dCtl.state; a.control = dCtl.control;
    a.order = c->dOrder.ptr; a.pcm = c->dPcm.ptr; a.result = c->dResult.ptr; a.state = nullptr;
    a.nSlots = plan.nCtl;

    c->done.assign(n, 0u);
    c->lastKernelMs = 0.0f; c->lastLaunches = 0;
    double tFill = 0, tRun = 0;
    unsigned int at = 0;                 // samples of the call behind us
    bool joined = false;                 // the pieces of a call in pieces are put together in dPcmJoin
    while (at < count) {
        const auto ta = now();
        unsigned int piece;
        if (pull_refill(p, count - at, &piece)) return -1;
        pull_fill(p, piece);
        const auto tb = now();
        tFill += ms(ta, tb);
        {
            std::lock_guard<std::mutex> lg(c->logMu);
            if (log_send(c)) return -1;
        }
        HIP_TRY(hipMemcpyAsync(c->dCtl.ptr, c->hCtl.ptr, p.ctl.bytes(), hipMemcpyHostToDevice, c->stream));
        a.maxSamples = piece;
#ifdef KLATT_STAMPS
        static unsigned long long* dStamps = nullptr;
        if (!dStamps) HIP_TRY(hipMalloc(&dStamps, 32 * 8));
        HIP_TRY(hipMemsetAsync(dStamps, 0, 32 * 8, c->stream));
        a.debug = plan.groups == 1 ? dStamps : nullptr;
#endif
        HIP_TRY(hipEventRecord(c->kernelStart, c->stream));
        if (pull_launch(p, a)) return -1;
        HIP_TRY(hipEventRecord(c->kernelStop, c->stream));
#ifdef KLATT_STAMPS
        if (a.debug) {
            unsigned long long h[32];
            HIP_TRY(hipMemcpyAsync(h, dStamps, sizeof h, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (int k = 0; k < 32; ++k) g_streamStamps[k] += h[k];
        }
#endif
        HIP_TRY(hipMemcpyAsync(c->hResult.ptr, c->dResult.ptr, (size_t)plan.nResults * sizeof(UttResult), hipMemcpyDeviceToHost, c->stream));
        if (piece < count || joined) {       // a call in pieces: this piece's columns into the joined rows
            if ((padded * n > c->dPcmJoin.cap && live_wait_exports(c, true)) || c->dPcmJoin.reserve(padded * n)) return -1;
            HIP_TRY(hipMemcpy2DAsync(c->dPcmJoin.ptr + at, padded * sizeof(int16_t), c->dPcm.ptr, padded * sizeof(int16_t), (size_t)piece * sizeof(int16_t), n,
                                     hipMemcpyDeviceToDevice, c->stream));
            joined = true;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        { std::lock_guard<std::mutex> lg(c->logMu); c->log.arrived(); }
        float kms = 0.0f;
        (void)hipEventElapsedTime(&kms, c->kernelStart, c->kernelStop);
        c->lastKernelMs += kms; c->lastLaunches++;
        if (pull_apply(p, piece)) return -1;
        at += piece;
        tRun += ms(tb, now());
    }
    const auto t2 = now();
    const int16_t* const pcm = joined ? c->dPcmJoin.ptr : c->dPcm.ptr;
    if (devicePcm) *devicePcm = pcm;
    if (deviceStride) *deviceStride = (long long)padded;
    size_t lastWithData = 0;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        produced[i] = (int)c->done[i];
        if (c->done[i]) { lastWithData = i; any = true; }
    }
    if (exportTo && live_export(c, pcm, padded, produced, n, *exportTo)) return -1;
    if (any && outs) {
        if (n == 1) {
            HIP_TRY(hipMemcpy(outs[0], pcm, (size_t)c->done[0] * sizeof(int16_t), hipMemcpyDeviceToHost));
        } else if (pull_hand_out(c, pcm, padded, lastWithData + 1, outs)) return -1;
    }
    if (trace)
        fprintf(stderr, "[speechPlayer/live] %d handles x %u in %d launch(es): control block + ring refill %.2f ms | log + upload + kernel (%.2f ms) + results %.2f ms | PCM to host %.2f ms | before %.2f ms\n",
                n, count, c->lastLaunches, tFill, c->lastKernelMs, tRun, ms(t2, now()), ms(t0, t2) - tFill - tRun);
    return 0;
}

// One bulk queue call (speechPlayer_queueFramesMany, _queueFramesManyDevice; speechPlayer_queueFrame is the host call with one handle
// and one frame): handle i is given frames frameStart[i] .. frameStart[i+1]-1 in order, the first of them after a purge when purge[i]
// is set (queue_frames).
struct QueueCall {
    const char* what = "";
    const speechPlayer_handle_t* handles = nullptr;
    int n = 0;
    const long long* frameStart = nullptr;
    const void* frames = nullptr;        // [nFrames][47] doubles in host memory (nullptr: every frame is NULL), or in device memory (onDevice)
    bool onDevice = false;
    const unsigned int* minDur = nullptr;
    const unsigned int* fadeDur = nullptr;
    const int* userIndex = nullptr;      // nullptr: -1
    const unsigned char* isNull = nullptr;
    const unsigned char* purge = nullptr;
    hipStream_t readyStream = nullptr;   // onDevice: the frames are ready once the work queued there so far has run (nullptr: now)
};

}  // namespace

// ==========================================================================================
// C-ABI: the reference's five entry points
// ==========================================================================================
extern "C" {

const char* speechPlayer_lastError(void) { return g_lastError.c_str(); }
// for the library's other translation units (frame_producer.cpp); not in the public headers
void speechPlayer_internal_setError(int code, const char* message)
{
    g_lastErrorCode = 0;
    set_error_code(code);
    set_error("%s", message ? message : "");
}
int speechPlayer_lastErrorCode(void) { return g_lastErrorCode; }

speechPlayer_handle_t speechPlayer_initialize(int sampleRate)
{
    begin_call();
    int dev = pick_device(-1);
    if (dev < 0) return nullptr;
    Stream* s = new Stream;
    s->sampleRate = sampleRate;
    s->mode = g_liveOptions.snapshot().mode;
    s->device = dev;
    if (stream_init_device(s)) { delete s; return nullptr; }
    std::lock_guard<std::mutex> g(g_tableMutex);
    for (size_t i = 0; i < g_streams.size(); ++i)
        if (!g_streams[i]) { g_streams[i] = s; s->id = i + 1; return reinterpret_cast<speechPlayer_handle_t>(i + 1); }
    g_streams.push_back(s);
    s->id = g_streams.size();
    return reinterpret_cast<speechPlayer_handle_t>(g_streams.size());
}

static int queue_frames(const QueueCall& q);

// The bulk call with one handle and one frame: one queue path (queue_frames).
void speechPlayer_queueFrame(speechPlayer_handle_t playerHandle, speechPlayer_frame_t* framePtr, unsigned int minFrameDuration,
                             unsigned int fadeDuration, int userIndex, bool purgeQueue)
{
    begin_call();
    static const long long one[2] = {0, 1};
    const unsigned char isNull = framePtr ? 0 : 1, purge = purgeQueue ? 1 : 0;
    QueueCall q;
    q.what = "speechPlayer_queueFrame"; q.handles = &playerHandle; q.n = 1; q.frameStart = one; q.frames = framePtr;
    q.minDur = &minFrameDuration; q.fadeDur = &fadeDuration; q.userIndex = &userIndex; q.isNull = &isNull; q.purge = &purge;
    (void)queue_frames(q);
}

int speechPlayer_synthesize(speechPlayer_handle_t playerHandle, unsigned int sampleCount, sample* sampleBuf)
{
    begin_call();
    Stream* s = lookup(playerHandle);
    if (!s) { set_error("speechPlayer_synthesize: invalid handle"); return 0; }
    std::lock_guard<std::mutex> g(s->mu);
    int produced = 0;
    sample* out = sampleBuf;
    if (streams_synthesize(&s, 1, sampleCount, &out, &produced)) return 0;
    return produced;
}

int speechPlayer_getLastIndex(speechPlayer_handle_t playerHandle)
{
    Stream* s = lookup(playerHandle);
    if (!s) return -1;
    return s->lastIndex;   // unlocked, as reference src/frame.cpp:117-119
}

void speechPlayer_terminate(speechPlayer_handle_t playerHandle)
{
    begin_call();
    Stream* s = nullptr;
    {
        uintptr_t id = reinterpret_cast<uintptr_t>(playerHandle) & 0xFFFFFFFFu;
        std::lock_guard<std::mutex> g(g_tableMutex);
        if (id == 0 || id > g_streams.size()) return;
        s = g_streams[id - 1];
        g_streams[id - 1] = nullptr;
    }
    if (!s) return;
    { std::lock_guard<std::mutex> g(s->mu); }   // let a call in flight finish
    if (LiveContext* c = s->context) {
        std::lock_guard<std::mutex> g(c->mu);
        ring_drop(c, s);                        // its entries in the log go nowhere
        c->freeSlots.push_back(s->slot);        // state block and ring are the next handle's (zeroed at its initialize, in stream order)
        if (g_liveOptions.snapshot().trim && hipSetDevice(s->device) == hipSuccess) arena_trim(c);
    }
    delete s;
}

// Additive: choose the handle's noise stream (default 0) and arithmetic mode.
int speechPlayer_setNoiseSeed(speechPlayer_handle_t playerHandle, unsigned int seed)
{
    begin_call();
    Stream* s = lookup(playerHandle);
    if (!s) return -1;
    std::lock_guard<std::mutex> g(s->mu);
    s->seed = seed;
    return 0;
}

// Additive: process-wide options.  "live_layout": which kernel advances live handles (1: stage-parallel, default; 0: lane kernel).
int speechPlayer_setGlobalOption(const char* name, int value)
{
    begin_call();
    // the "live_*" options: klatt_live.h says what each takes and how it is clamped
    const int live = g_liveOptions.set(name, value);
    if (live < 0) { set_error("live_mode: 0 or 1"); return -1; }
    if (live == 0) {
        if (!strcmp(name, "live_trim") && value) {      // ... and now, on devices where no handle lives
            std::vector<LiveContext*> all;
            { std::lock_guard<std::mutex> g(g_liveMutex); all = g_live; }
            for (size_t dev = 0; dev < all.size(); ++dev)
                if (all[dev] && hipSetDevice((int)dev) == hipSuccess) { std::lock_guard<std::mutex> g(all[dev]->mu); arena_trim(all[dev]); }
        }
        return 0;
    }
    // "plan_hash_bits" (tests): the track planner looks at this many bits of a frame's 128-bit shape hash (default 128).  With few bits
    // different frames collide for certain, which is how the tests reach the verification of hashed shapes (klatt_verify_shared) and the
    // fall-back behind it; the PCM must not change.
    if (name && !strcmp(name, "plan_hash_bits")) {
        const int bits = value < 0 ? 0 : (value > 128 ? 128 : value);
        g_planHashMask[0].store(bits >= 64 ? ~0ull : (bits == 0 ? 0ull : ((1ull << bits) - 1ull)), std::memory_order_relaxed);
        g_planHashMask[1].store(bits >= 128 ? ~0ull : (bits <= 64 ? 0ull : ((1ull << (bits - 64)) - 1ull)), std::memory_order_relaxed);
        return 0;
    }
    set_error("unknown global option %s", name ? name : "(null)");
    return -1;
}

// Additive: advance many live handles together -- one kernel launch, one handle per wavefront lane.
// Equivalent to calling speechPlayer_synthesize(handles[i], sampleCount, sampleBufs[i]) for every i;
// produced[i] receives each call's return value.  Handles must be distinct and share a sample rate.
static int synthesize_many(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, sample** sampleBufs, int* produced,
                           const int16_t** devicePcm, long long* deviceStride, const char* what, const LiveExport* exportTo);

int speechPlayer_synthesizeMany(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, sample** sampleBufs, int* produced)
{
    begin_call();
    if (nHandles > 0 && !sampleBufs) { set_error("speechPlayer_synthesizeMany: bad arguments"); return -1; }
    return synthesize_many(handles, nHandles, sampleCount, sampleBufs, produced, nullptr, nullptr, "speechPlayer_synthesizeMany", nullptr);
}

// The same with the PCM left in HBM: handle i's samples start at *devicePcm + i * *rowStride (valid until the next live call
// on that device).  For consumers on the GPU, and for measuring the engine without the PCIe copy of the PCM.
int speechPlayer_synthesizeManyDevice(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, const sample** devicePcm,
                                      long long* rowStride, int* produced)
{
    begin_call();
    if (!devicePcm || !rowStride) { set_error("speechPlayer_synthesizeManyDevice: bad arguments"); return -1; }
    const int16_t* p = nullptr;
    const int rc = synthesize_many(handles, nHandles, sampleCount, nullptr, produced, &p, rowStride, "speechPlayer_synthesizeMany", nullptr);
    *devicePcm = reinterpret_cast<const sample*>(p);
    return rc;
}

static bool device_range(const void* p, size_t bytes, int device, size_t align, const char* what);

// The same with the rows written to caller-owned device memory on the caller's stream (live_export).
int speechPlayer_synthesizeManyExport(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, void* deviceOut, int format,
                                      long long rowStride, void* stream, int* produced)
{
    begin_call();
    const char* what = "speechPlayer_synthesizeManyExport";
    if (refuse_timing_only(what)) return -1;
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    if (rowStride == 0) rowStride = sampleCount;
    if (rowStride < (long long)sampleCount) { set_error("%s: rowStride %lld is below sampleCount %u", what, rowStride, sampleCount); return -1; }
    if (nHandles > 0 && rowStride > (1ll << 50) / nHandles) { set_error("%s: %d rows of %lld elements", what, nHandles, rowStride); return -1; }
    const LiveExport x{deviceOut, format, rowStride, static_cast<hipStream_t>(stream)};
    const int rc = synthesize_many(handles, nHandles, sampleCount, nullptr, produced, nullptr, nullptr, what, &x);
    if (rc == 0 && sampleCount == 0 && nHandles > 0 && rowStride > 0)       // nothing pulled (no pull buffer): the rows are zeros
        HIP_TRY(hipMemsetAsync(deviceOut, 0, (size_t)nHandles * rowStride * (format ? sizeof(float) : sizeof(int16_t)), x.stream));
    return rc;
}

// The export's memory: device memory of the handles' device, aligned to the element, holding their rows.
static int live_export_check(const std::vector<Stream*>& ss, const LiveExport& x, const char* what)
{
    const int device = ss[0]->device;
    for (size_t i = 1; i < ss.size(); ++i)
        if (ss[i]->device != device) { set_error("%s: handles on devices %d and %d", what, device, ss[i]->device); return -1; }
    const long long elements = (long long)ss.size() * x.rowStride;
    if (elements == 0) return 0;
    if (!x.out) { set_error("%s: no output buffer", what); return -1; }
    if (hipSetDevice(device) != hipSuccess) { set_error_code(SPEECHPLAYER_ERR_HIP); set_error("%s: cannot select device %d", what, device); return -1; }
    const size_t elSize = x.format ? sizeof(float) : sizeof(int16_t);
    return device_range(x.out, (size_t)elements * elSize, device, elSize, what) ? 0 : -1;
}

// Duration in milliseconds of the last live-handle launch on `device` (HIP events around the kernel on its stream).
float speechPlayer_lastLiveKernelMs(int device)
{
    std::lock_guard<std::mutex> g(g_liveMutex);
    return (device >= 0 && device < (int)g_live.size() && g_live[device]) ? g_live[device]->lastKernelMs : -1.0f;
}

// Kernel launches the last live call on `device` took: 1, unless it went in pieces (a handle with more frames queued than its ring holds).
int speechPlayer_lastLiveLaunches(int device)
{
    std::lock_guard<std::mutex> g(g_liveMutex);
    return (device >= 0 && device < (int)g_live.size() && g_live[device]) ? g_live[device]->lastLaunches : -1;
}

// Look the handles up (ss, in the call's order) and sort them into the lock order (order: ascending creation; no deadlock between
// concurrent calls); an invalid handle and a handle listed twice are errors.
static int lookup_handles(const speechPlayer_handle_t* handles, int n, std::vector<Stream*>& ss, std::vector<Stream*>& order, const char* what)
{
    ss.resize((size_t)n);
    bool ascending = true;
    {
        std::lock_guard<std::mutex> g(g_tableMutex);
        for (int i = 0; i < n; ++i) {
            ss[i] = lookup_locked(handles[i]);
            if (!ss[i]) { set_error("%s: invalid handle at %d", what, i); return -1; }
            if (i && ss[i]->id <= ss[i - 1]->id) ascending = false;
        }
    }
    order = ss;
    if (!ascending) std::sort(order.begin(), order.end(), [](Stream* x, Stream* y) { return x->id < y->id; });
    for (size_t i = 1; i < order.size(); ++i)
        if (order[i] == order[i - 1]) { set_error("%s: handle listed twice", what); return -1; }
    return 0;
}

static int synthesize_many(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, sample** sampleBufs, int* produced,
                           const int16_t** devicePcm, long long* deviceStride, const char* what, const LiveExport* exportTo)
{
    if (nHandles < 0 || (nHandles > 0 && (!handles || !produced))) { set_error("%s: bad arguments", what); return -1; }
    std::vector<Stream*> ss, order;
    if (lookup_handles(handles, nHandles, ss, order, what)) return -1;
    if (exportTo && nHandles > 0 && live_export_check(ss, *exportTo, what)) return -1;
    for (Stream* s : order) s->mu.lock();
    const int rc = streams_synthesize(ss.data(), nHandles, sampleCount, sampleBufs, produced, devicePcm, deviceStride, exportTo);
    for (Stream* s : order) s->mu.unlock();
    return rc;
}

// ------------------------------------------------------------------------------------------
// Bulk queueing: speechPlayer_queueFramesMany, _queueFramesManyDevice (and speechPlayer_queueFrame, the host call with one frame)
// ------------------------------------------------------------------------------------------
// Everything is checked before anything is queued: a refused call changes no handle.
static int queue_check(const QueueCall& q, std::vector<Stream*>& ss, std::vector<Stream*>& order)
{
    if (q.n < 0 || (q.n > 0 && (!q.handles || !q.frameStart))) { set_error("%s: bad arguments", q.what); return -1; }
    if (q.n == 0) return 0;
    if (q.frameStart[0] != 0) { set_error("%s: frameStart[0] = %lld (frameStart runs from 0)", q.what, q.frameStart[0]); return -1; }
    for (int i = 0; i < q.n; ++i) {
        if (q.frameStart[i + 1] < q.frameStart[i]) {
            set_error("%s: frameStart decreases at %d (%lld -> %lld)", q.what, i + 1, q.frameStart[i], q.frameStart[i + 1]);
            return -1;
        }
        if (q.purge && q.purge[i] && q.frameStart[i + 1] == q.frameStart[i]) { set_error("%s: purge[%d] is set on a handle given no frames", q.what, i); return -1; }
    }
    const long long nF = q.frameStart[q.n];
    if (nF > (1ll << 48)) { set_error("%s: frameStart[%d] = %lld", q.what, q.n, nF); return -1; }
    if (nF > 0 && (!q.minDur || !q.fadeDur)) { set_error("%s: no durations", q.what); return -1; }
    if (nF > 0 && !q.frames) {           // (host frames may be absent when every frame is NULL)
        long long k = 0;
        if (!q.onDevice && q.isNull) while (k < nF && q.isNull[k]) ++k;
        if (k < nF) { set_error("%s: no frames", q.what); return -1; }
    }
    if (lookup_handles(q.handles, q.n, ss, order, q.what)) return -1;
    if (q.onDevice && nF > 0) {
        const int device = ss[0]->device;
        for (int i = 1; i < q.n; ++i)
            if (ss[i]->device != device) { set_error("%s: handles on devices %d and %d", q.what, device, ss[i]->device); return -1; }
        if (hipSetDevice(device) != hipSuccess) { set_error_code(SPEECHPLAYER_ERR_HIP); set_error("%s: cannot select device %d", q.what, device); return -1; }
        if (!device_range(q.frames, (size_t)nF * sizeof(speechPlayer_frame_t), device, 8, q.what)) return -1;
    }
    return 0;
}

static FrameMeta queue_meta(const QueueCall& q, long long k)
{
    FrameMeta m;
    m.minSamples = q.minDur[k];
    m.fadeSamples = std::max(q.fadeDur[k], 1u);          // reference src/speechPlayer.cpp:36
    m.userIndex = q.userIndex ? q.userIndex[k] : -1;
    m.flags = (!q.frames || (q.isNull && q.isNull[k])) ? FRAME_NULL : 0u;
    return m;
}

// The handles' mutexes held.  Every frame into its ring by way of the pinned log, or into the host queue (FrameQueue::takes_now).
static int queue_host(const QueueCall& q, Stream* const* ss)
{
    const double* frames = static_cast<const double*>(q.frames);
    for (int i = 0; i < q.n; ++i) {
        const long long k0 = q.frameStart[i], k1 = q.frameStart[i + 1];
        if (k0 == k1) continue;
        Stream* s = ss[i];
        LiveContext* const c = s->context;
        if (q.purge && q.purge[i]) stream_purge(c, s);
        bool logged = false;
        for (long long k = k0; k < k1; ++k) {
            const FrameMeta meta = queue_meta(q, k);
            const double* p = (meta.flags & FRAME_NULL) ? nullptr : frames + k * kNumParams;
            if (!s->q.takes_now()) { s->q.push_host(p, meta); continue; }
            if (log_append(c, s, p, meta, s->q.claim(meta), false)) { s->q.unclaim(); return -1; }
            logged = true;
        }
        if (!logged) continue;
        bool eager;
        { std::lock_guard<std::mutex> lg(c->logMu); eager = c->log.waiting() >= kLogEager; }
        if (eager && c->mu.try_lock()) {                 // no pull is running: the log need not wait for the next one
            std::lock_guard<std::mutex> lg(c->logMu);
            if (hipSetDevice(s->device) == hipSuccess) (void)log_send(c);
            c->mu.unlock();
        }
    }
    return 0;
}

// The handles' mutexes held; one device.  The same choice per frame as queue_host.  A ring frame is placed by live_place from the
// caller's memory (the log is sent first: one stream carries every frame in queue order); the rows of host-queue frames are gathered
// on the device (klatt_gather_frames) and downloaded.  Returns once the caller's memory has been read.
static int queue_device(const QueueCall& q, Stream* const* ss)
{
    const double* frames = static_cast<const double*>(q.frames);
    const int device = ss[0]->device;
    LiveContext* const c = ss[0]->context;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(device));
    const long long nF = q.frameStart[q.n];
    const size_t placeCap = (size_t)std::min<long long>(nF, (long long)q.n * kRing);      // a call fills a ring at most once
    if (c->hPlace.reserve(placeCap) || c->dPlace.reserve(c->hPlace.cap) || c->hGatherIdx.reserve((size_t)nF) || c->dGatherIdx.reserve(c->hGatherIdx.cap))
        return -1;
    if (q.readyStream) {
        HIP_TRY(hipEventRecord(c->inputReady, q.readyStream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->inputReady, 0));
    }
    {
        std::lock_guard<std::mutex> lg(c->logMu);
        if (log_send(c)) return -1;
    }
    struct Fill { Stream* s; size_t at; };               // a host-queue frame whose values the download brings
    std::vector<Fill> fill;
    size_t nPlace = 0, nGather = 0;
    for (int i = 0; i < q.n; ++i) {
        const long long k0 = q.frameStart[i], k1 = q.frameStart[i + 1];
        if (k0 == k1) continue;
        Stream* s = ss[i];
        if (q.purge && q.purge[i]) stream_purge(c, s);
        for (long long k = k0; k < k1; ++k) {
            const FrameMeta meta = queue_meta(q, k);
            const bool null = (meta.flags & FRAME_NULL) != 0;
            if (s->q.takes_now()) {
                LivePlace& p = c->hPlace.ptr[nPlace++];
                p.meta = meta; p.row = null ? -1 : k; p.pad = 0;
                p.target = s->slot * kRing + s->q.claim(meta);
            } else {
                s->q.push_host(nullptr, meta);
                if (!null) { c->hGatherIdx.ptr[nGather++] = k; fill.push_back(Fill{s, s->q.overflow.size() - 1}); }
            }
        }
    }
    if (nGather && (c->hGatherRows.reserve(nGather * kNumParams) || c->dGatherRows.reserve(c->hGatherRows.cap))) return -1;
    if (nPlace) {
        HIP_TRY(hipMemcpyAsync(c->dPlace.ptr, c->hPlace.ptr, nPlace * sizeof(LivePlace), hipMemcpyHostToDevice, c->stream));
        const unsigned grid = (unsigned)std::min<size_t>((nPlace + 3) / 4, (size_t)1 << 20);
        hipLaunchKernelGGL(live_place, dim3(grid), dim3(256), 0, c->stream, frames, c->dPlace.ptr, (long long)nPlace, c->dRingFrames.ptr, c->dRingMeta.ptr);
        HIP_TRY(hipGetLastError());
    }
    if (nGather) {
        HIP_TRY(hipMemcpyAsync(c->dGatherIdx.ptr, c->hGatherIdx.ptr, nGather * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        const unsigned grid = (unsigned)std::min<size_t>((nGather * kNumParams + 255) / 256, (size_t)1 << 16);
        hipLaunchKernelGGL(klatt_gather_frames, dim3(grid), dim3(256), 0, c->stream, frames, c->dGatherIdx.ptr, (long long)nGather, c->dGatherRows.ptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->hGatherRows.ptr, c->dGatherRows.ptr, nGather * kNumParams * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));            // the caller's memory has been read
    { std::lock_guard<std::mutex> lg(c->logMu); c->log.arrived(); }
    for (size_t j = 0; j < nGather; ++j) memcpy(fill[j].s->q.overflow[fill[j].at].p, c->hGatherRows.ptr + j * kNumParams, kNumParams * sizeof(double));
    return 0;
}

static int queue_frames(const QueueCall& q)
{
    std::vector<Stream*> ss, order;
    if (queue_check(q, ss, order)) return -1;
    if (q.n == 0 || q.frameStart[q.n] == 0) return 0;
    for (Stream* s : order) s->mu.lock();
    const int rc = q.onDevice ? queue_device(q, ss.data()) : queue_host(q, ss.data());
    for (Stream* s : order) s->mu.unlock();
    return rc;
}

int speechPlayer_queueFramesMany(const speechPlayer_handle_t* handles, int nHandles, const long long* frameStart, const speechPlayer_frame_t* frames,
                                 const unsigned int* minFrameDuration, const unsigned int* fadeDuration, const int* userIndex,
                                 const unsigned char* isNull, const unsigned char* purge)
{
    begin_call();
    QueueCall q;
    q.what = "speechPlayer_queueFramesMany"; q.handles = handles; q.n = nHandles; q.frameStart = frameStart; q.frames = frames;
    q.minDur = minFrameDuration; q.fadeDur = fadeDuration; q.userIndex = userIndex; q.isNull = isNull; q.purge = purge;
    return queue_frames(q);
}

int speechPlayer_queueFramesManyDevice(const speechPlayer_handle_t* handles, int nHandles, const long long* frameStart,
                                       const speechPlayer_frame_t* deviceFrames, const unsigned int* minFrameDuration,
                                       const unsigned int* fadeDuration, const int* userIndex, const unsigned char* isNull,
                                       const unsigned char* purge, void* readyStream)
{
    begin_call();
    QueueCall q;
    q.what = "speechPlayer_queueFramesManyDevice"; q.handles = handles; q.n = nHandles; q.frameStart = frameStart; q.frames = deviceFrames;
    q.onDevice = true; q.minDur = minFrameDuration; q.fadeDur = fadeDuration; q.userIndex = userIndex; q.isNull = isNull; q.purge = purge;
    q.readyStream = static_cast<hipStream_t>(readyStream);
    return queue_frames(q);
}

int speechPlayer_handleDevice(speechPlayer_handle_t handle)
{
    begin_call();
    Stream* s = lookup(handle);
    if (!s) { set_error("speechPlayer_handleDevice: invalid handle"); return -1; }
    return s->device;
}

// ==========================================================================================
// C-ABI: batch
// ==========================================================================================
speechPlayer_batch_t speechPlayer_batch_create(int sampleRate, int device)
{
    begin_call();
    int dev = pick_device(device);
    if (dev < 0) return nullptr;
    Batch* b = new Batch;
    b->sampleRate = sampleRate;
    b->device = dev;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) b->cus = prop.multiProcessorCount; }
    bool ok = hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&b->forkEvent, hipEventDisableTiming) == hipSuccess &&
              hipStreamCreateWithFlags(&b->copyStream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&b->denseReady, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&b->copyDone, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&b->inputReady, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&b->pcmReady, hipEventDisableTiming) == hipSuccess;
    for (auto& s : b->exportSlot) ok = ok && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
    for (auto& s : b->trackSlot) ok = ok && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t* e : {&b->setDone, &b->setCopied, &b->timelineReady, &b->pitchOrder.done, &b->sourceOrder.done, &b->resampleOrder.done, &b->bankOrder.done}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    { const char* e = getenv("SPEECHPLAYER_TRACKS"); if (e) b->tracks = atoi(e) ? 1 : 0; }
    { const char* e = getenv("SPEECHPLAYER_DIRECT"); if (e) b->direct = std::min(2, std::max(0, atoi(e))); }
    { const char* e = getenv("SPEECHPLAYER_DIRECT_LEAN"); if (e) b->directLean = std::min(1, std::max(-1, atoi(e))); }
    for (int i = 0; i < 6 && ok; ++i)
        ok = hipStreamCreateWithFlags(&b->side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&b->join[i], hipEventDisableTiming) == hipSuccess;
    { const char* e = getenv("SPEECHPLAYER_QUIET_LAST"); if (e) b->quietLast = atoi(e) ? 1 : 0; }
    if (!ok) {
        set_error("cannot create a stream on device %d", dev);
        speechPlayer_batch_destroy(b);
        return nullptr;
    }
    return b;
}

void speechPlayer_batch_destroy(speechPlayer_batch_t batch)
{
    Batch* b = static_cast<Batch*>(batch);
    if (!b) return;
    (void)hipSetDevice(b->device);
    while (!b->stages.empty()) stage_release(b->stages.back());      // (its signal stages go with it)
    (void)sync_exports(b);      // (exports on the callers' streams may still read the pool)
    for (auto& s : b->exportSlot) {
        if (s.done) (void)hipEventDestroy(s.done);
        s.host.release(); s.dev.release();
    }
    (void)settle_track_exports(b, true);
    for (auto& s : b->trackSlot) {
        if (s.done) (void)hipEventDestroy(s.done);
        s.host.release(); s.dev.release();
    }
    for (hipEvent_t e : {b->setDone, b->setCopied, b->timelineReady, b->pitchOrder.done, b->sourceOrder.done, b->resampleOrder.done, b->bankOrder.done}) if (e) (void)hipEventDestroy(e);
    b->dListStart.release(); b->dTimeline.release(); b->dPitch.release(); b->dLabels.release(); b->dUnitFirst.release();
    b->dSource.release(); b->dEpochs.release(); b->dEpochCount.release(); b->dResample.release(); b->dBank.release();
    if (b->inputReady) (void)hipEventDestroy(b->inputReady);
    if (b->pcmReady) (void)hipEventDestroy(b->pcmReady);
    b->dShapeIdx.release(); b->dShapeRows.release();
    if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
    for (int i = 0; i < 6; ++i) {
        if (b->side[i]) { (void)hipStreamSynchronize(b->side[i]); (void)hipStreamDestroy(b->side[i]); }
        if (b->join[i]) (void)hipEventDestroy(b->join[i]);
    }
    if (b->forkEvent) (void)hipEventDestroy(b->forkEvent);
    if (b->copyStream) { (void)hipStreamSynchronize(b->copyStream); (void)hipStreamDestroy(b->copyStream); }
    if (b->denseReady) (void)hipEventDestroy(b->denseReady);
    if (b->copyDone) (void)hipEventDestroy(b->copyDone);
    b->dDense.release(); b->dDenseStart.release(); b->dFacts.release(); b->hFacts.release();
    b->dRecords.release(); b->dShapeTable.release(); b->dRep.release(); b->dMismatch.release();
    b->dFrames.release(); b->dMeta.release(); b->dUtt.release(); b->dOrder.release(); b->dPcm.release(); b->dResult.release();
    b->dFloat.release(); b->dDebug.release(); b->dDigest.release(); b->bounce.release(); b->dDeadWaves.release(); b->dPresent2.release();
    b->dFlatRef.release(); b->dSourceRef.release(); b->dJobs.release(); b->dShapes.release(); b->dTrack.release();
    b->dDirectJobs.release(); b->dDirectFirst.release(); b->dDirectHdr.release(); b->dDirectRec.release();
    delete b;
}

int speechPlayer_batch_setOption(speechPlayer_batch_t batch, const char* name, int value)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || !name) return -1;
    if (!strcmp(name, "mode")) {
        if (value != MODE_EXACT && value != MODE_FAST) { set_error("mode %d not available", value); return -1; }
        b->mode = value;
        return 0;
    }
    if (!strcmp(name, "sort")) { b->sortByLength = value ? 1 : 0; return 0; }
    if (!strcmp(name, "quiet_last")) { b->quietLast = value ? 1 : 0; return 0; }      // read by every launch (batch_launch)
    if (!strcmp(name, "layout")) { b->layout = value < 0 ? -1 : (value > 2 ? 1 : value); return 0; }
    // tracks: planned by setUtterances (set the option before it), used by the stage-parallel layouts
    if (!strcmp(name, "tracks")) { b->tracks = value ? 1 : 0; return 0; }
    if (!strcmp(name, "dead_terms")) { b->deadTerms = value ? 1 : 0; return 0; }
    if (!strcmp(name, "track_budget_mb")) { b->trackBudgetMB = value < 0 ? 0 : value; return 0; }
    // direct: read by setUtterances (set the option before it); 0 never, 1 unless the lanes are time-aligned (default), 2 always
    if (!strcmp(name, "direct")) { b->direct = value < 0 ? 0 : (value > 2 ? 2 : value); return 0; }
    // direct_lean: the direct stages two workgroups to a CU (1), one (0), or the engine's choice (-1, default); same PCM in MODE_EXACT
    if (!strcmp(name, "direct_lean")) { b->directLean = value < 0 ? -1 : (value ? 1 : 0); return 0; }
    // pitch_table_mb: read by speechPlayer_batch_exportTracks (the voicePitch table of an export; a larger one proceeds in pieces)
    if (!strcmp(name, "pitch_table_mb")) { b->pitchBudgetMB = value < 1 ? 1 : value; return 0; }
    // source_table_mb: read by speechPlayer_batch_exportSource (the step table of an export; a larger one proceeds in pieces)
    if (!strcmp(name, "source_table_mb")) { b->sourceBudgetMB = value < 1 ? 1 : value; return 0; }
    // source_lane_lists: a source walk over at least this many frame lists runs one lane per list instead of one wavefront (same bits)
    if (!strcmp(name, "source_lane_lists")) { b->sourceLaneLists = value < 1 ? 1 : value; return 0; }
    set_error("unknown option %s", name);
    return -1;
}

// What a set call describes: `nLists` frame lists -- as full frames (frames, durations, marks, silences) or as records over a shape table
// -- and `nUtt` utterances, each speaking one list (listOf == nullptr: utterance u speaks list u).  speechPlayer_batch_setUtterances is
// the case "every utterance its own list, full frames".
struct SetInput {
    long long nLists = 0;
    const long long* listStart = nullptr;
    const speechPlayer_frame_t* frames = nullptr;
    const unsigned int* minDur = nullptr;
    const unsigned int* fadeDur = nullptr;
    const int* userIndex = nullptr;
    const unsigned char* isNull = nullptr;
    const speechPlayer_frameRecord_t* records = nullptr;
    long long nShapes = 0;
    const speechPlayer_frame_t* shapes = nullptr;
    long long nUtt = 0;
    const unsigned int* listOf = nullptr;
    const unsigned int* seeds = nullptr;
    const double* deviceFrames = nullptr;   // speechPlayer_batch_setUtterancesDevice: the frames in device memory of the batch's device
    hipStream_t readyStream = nullptr;      // ... ready there once this stream's work queued so far is done (nullptr: ready now)
    const speechPlayer_frameLabel_t* labels = nullptr;      // speechPlayer_batch_setRecordsLabelled: one per list frame
    bool noTracks = false;       // the second attempt of a batch whose shared shapes failed their verification
};
static_assert(sizeof(speechPlayer_frameRecord_t) == sizeof(FrameRecord), "record layout");
static_assert(sizeof(speechPlayer_frameLabel_t) == sizeof(FrameLabel), "label layout");
static_assert(SPEECHPLAYER_LABEL_GAP == kLabelGap && SPEECHPLAYER_LABEL_PUFF == kLabelPuff && SPEECHPLAYER_ALIGN_COLUMNS == kAlignColumns &&
              SPEECHPLAYER_UNIT_COLUMNS == kUnitColumns, "alignment constants");

static void batch_clear(Batch* b)
{
    b->nUtt = 0; b->nFrames = 0; b->nFramesSpoken = 0; b->nLists = 0; b->nSlots = 0; b->nQuiet = 0; b->nNoNasal = 0; b->nNoNasalUtt = 0; b->totalSamples = 0; b->poolSamples = 0;
    b->nTracked = 0; b->nTrackedUtt = 0; b->nJobs = 0; b->trackEntries = 0; b->nDirect = 0; b->nDirectUtt = 0; b->nDirectFrames = 0; b->directAligned = false;
    b->lens.clear(); b->outStart.assign(1, 0); b->results.clear(); b->resultsFresh = false; b->floatFresh = false;
    b->uttFrameStart.clear(); b->uttFrames.clear(); b->uttList.clear(); b->uttSeed.clear(); b->timelineFresh = false; b->epochFresh = false;
    b->hasLabels = false; b->listUnits.clear();
}

static int batch_set(Batch* b, const SetInput& in);

static int batch_set_guarded(const char* what, speechPlayer_batch_t batch, const SetInput& in)
{
    begin_call();
    try {       // nothing may throw across the C ABI (host allocations of a large batch; the planning threads)
        return batch_set(static_cast<Batch*>(batch), in);
    } catch (const std::exception& e) {
        set_error("%s: %s", what, e.what());
        return -1;
    }
}

int speechPlayer_batch_setUtterances(speechPlayer_batch_t batch, long long nUtterances, const long long* frameStart,
                                     const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration,
                                     const unsigned int* fadeDuration, const int* userIndex, const unsigned char* isNull,
                                     const unsigned int* noiseSeed)
{
    SetInput in;
    in.nLists = nUtterances; in.listStart = frameStart; in.frames = frames; in.minDur = minFrameDuration; in.fadeDur = fadeDuration;
    in.userIndex = userIndex; in.isNull = isNull; in.nUtt = nUtterances; in.seeds = noiseSeed;
    return batch_set_guarded("setUtterances", batch, in);
}

// Is [p, p + bytes) device memory of `device`, inside one allocation, aligned to `align`?  (A kernel never runs on a pointer the
// runtime does not report as device memory: host memory, page-locked or not, managed memory and unknown pointers are refused.)
static bool device_range(const void* p, size_t bytes, int device, size_t align, const char* what)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: %p is not memory the HIP runtime knows (host memory?)", what, p);
        return false;
    }
    if (a.type != hipMemoryTypeDevice) { set_error("%s: %p is not device memory (memory type %d)", what, p, (int)a.type); return false; }
    if (a.device != device) { set_error("%s: %p is memory of device %d, the batch's is %d", what, p, a.device, device); return false; }
    if (reinterpret_cast<uintptr_t>(p) % align) { set_error("%s: %p is not %zu-byte aligned", what, p, align); return false; }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: the allocation that holds %p is unknown to the HIP runtime", what, p);
        return false;
    }
    if ((size_t)(static_cast<const char*>(p) - static_cast<const char*>(base)) + bytes > size) {
        set_error("%s: %zu bytes from %p run past the end of their allocation (%zu bytes from %p)", what, bytes, p, size, base);
        return false;
    }
    return true;
}

int speechPlayer_batch_setUtterancesDevice(speechPlayer_batch_t batch, long long nUtterances, const long long* frameStart,
                                           const speechPlayer_frame_t* deviceFrames, const unsigned int* minFrameDuration,
                                           const unsigned int* fadeDuration, const int* userIndex, const unsigned char* isNull,
                                           const unsigned int* noiseSeed, void* readyStream)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || nUtterances < 0 || !frameStart) { set_error("setUtterancesDevice: bad arguments"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { set_error_code(SPEECHPLAYER_ERR_HIP); set_error("setUtterancesDevice: cannot select device %d", b->device); return -1; }
    const long long nF = frameStart[nUtterances];
    if (nF < 0 || nF > (1ll << 48)) { set_error("setUtterancesDevice: frameStart[%lld] = %lld", nUtterances, nF); return -1; }
    if (nF > 0 && !deviceFrames) { set_error("setUtterancesDevice: no frames"); return -1; }
    if (nF > 0 && !device_range(deviceFrames, (size_t)nF * sizeof(speechPlayer_frame_t), b->device, 8, "setUtterancesDevice")) return -1;
    SetInput in;
    in.nLists = nUtterances; in.listStart = frameStart; in.minDur = minFrameDuration; in.fadeDur = fadeDuration;
    in.userIndex = userIndex; in.isNull = isNull; in.nUtt = nUtterances; in.seeds = noiseSeed;
    in.deviceFrames = reinterpret_cast<const double*>(deviceFrames); in.readyStream = static_cast<hipStream_t>(readyStream);
    return batch_set_guarded("setUtterancesDevice", batch, in);
}

int speechPlayer_batch_setUtterancesShared(speechPlayer_batch_t batch, long long nLists, const long long* listStart,
                                           const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
                                           const int* userIndex, const unsigned char* isNull, long long nUtterances, const unsigned int* listOf,
                                           const unsigned int* noiseSeed)
{
    SetInput in;
    in.nLists = nLists; in.listStart = listStart; in.frames = frames; in.minDur = minFrameDuration; in.fadeDur = fadeDuration;
    in.userIndex = userIndex; in.isNull = isNull; in.nUtt = nUtterances; in.listOf = listOf; in.seeds = noiseSeed;
    return batch_set_guarded("setUtterancesShared", batch, in);
}

// A batch of records over a shape table, with labels or without: `what` is the entry point's name in the messages.
static int batch_set_records(const char* what, speechPlayer_batch_t batch, long long nShapes, const speechPlayer_frame_t* shapes, long long nLists,
                             const long long* listStart, const speechPlayer_frameRecord_t* records, const speechPlayer_frameLabel_t* labels,
                             long long nUtterances, const unsigned int* listOf, const unsigned int* noiseSeed)
{
    SetInput in;
    in.nLists = nLists; in.listStart = listStart; in.records = records; in.nShapes = nShapes; in.shapes = shapes;
    in.nUtt = nUtterances; in.listOf = listOf; in.seeds = noiseSeed; in.labels = labels;
    if (nShapes < 0 || (nShapes > 0 && !shapes)) { begin_call(); set_error("%s: bad shape table", what); return -1; }
    if (!records && nLists > 0 && listStart && listStart[nLists] > 0) { begin_call(); set_error("%s: no records", what); return -1; }
    static const speechPlayer_frameRecord_t none = {0.0, 0.0, SPEECHPLAYER_RECORD_SILENCE, 0u, 0u, -1};
    if (!in.records) in.records = &none;      // (an empty batch: the record path all the same)
    return batch_set_guarded(what, batch, in);
}

int speechPlayer_batch_setRecords(speechPlayer_batch_t batch, long long nShapes, const speechPlayer_frame_t* shapes,
                                  long long nLists, const long long* listStart, const speechPlayer_frameRecord_t* records,
                                  long long nUtterances, const unsigned int* listOf, const unsigned int* noiseSeed)
{
    return batch_set_records("setRecords", batch, nShapes, shapes, nLists, listStart, records, nullptr, nUtterances, listOf, noiseSeed);
}

int speechPlayer_batch_setRecordsLabelled(speechPlayer_batch_t batch, long long nShapes, const speechPlayer_frame_t* shapes,
                                          long long nLists, const long long* listStart, const speechPlayer_frameRecord_t* records,
                                          const speechPlayer_frameLabel_t* labels, long long nUtterances, const unsigned int* listOf,
                                          const unsigned int* noiseSeed)
{
    return batch_set_records(labels ? "setRecordsLabelled" : "setRecords", batch, nShapes, shapes, nLists, listStart, records, labels, nUtterances, listOf, noiseSeed);
}

int speechPlayer_batch_hasLabels(speechPlayer_batch_t batch) { return batch ? (static_cast<Batch*>(batch)->hasLabels ? 1 : 0) : -1; }

// Frames in device memory (speechPlayer_batch_setUtterancesDevice) and the track planner: one frame per distinct (masked) shape hash
// stands for all frames of that hash (shape_table_rows, klatt_trackplan.h).  Their rows are gathered on the device
// (klatt_gather_frames) and downloaded: a few hundred rows for speech, instead of the frames.
static int device_shape_table(Batch* b, long long nL, const long long* listStart, const FrameMeta* meta, const FrameFacts* facts,
                              const unsigned char* eligible, HashMask mask, RawVector<uint32_t>& rowOf, std::vector<long long>& rep, std::vector<double>& rows)
{
    shape_table_rows(nL, listStart, meta, facts, eligible, mask, rowOf, rep);
    const size_t nRows = rep.size();
    rows.assign(nRows * kNumParams, 0.0);
    if (nRows == 0) return 0;
    if (b->dShapeIdx.reserve(nRows) || b->dShapeRows.reserve(nRows * kNumParams)) return -1;
    HIP_TRY(hipMemcpyAsync(b->dShapeIdx.ptr, rep.data(), nRows * sizeof(long long), hipMemcpyHostToDevice, b->copyStream));
    const unsigned grid = (unsigned)std::min<long long>(((long long)nRows * kNumParams + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(klatt_gather_frames, dim3(grid), dim3(256), 0, b->copyStream, b->dFrames.ptr, b->dShapeIdx.ptr, (long long)nRows, b->dShapeRows.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rows.data(), b->dShapeRows.ptr, nRows * kNumParams * sizeof(double), hipMemcpyDeviceToHost, b->copyStream));
    HIP_TRY(hipStreamSynchronize(b->copyStream));
    return 0;
}

// The first bad index the threads of a parallel_ranges come across (-1: none).
struct FirstBad {
    std::atomic<long long> at{-1};
    void mark(long long i) { long long none = -1; at.compare_exchange_strong(none, i); }
    long long get() const { return at.load(); }
};

// Per-frame work arrays are kept between calls (per calling thread): a fresh 25-50 MB vector costs its page faults on first touch
// and its unmapping on release -- together ~15 ms of a 65 ms call for BASELINE configs[2].  Every element is written before it
// is read.  (Released again when a batch was very large: kScratchKeepFrames.)
// (RawVector: resize() leaves new elements uninitialised, so a fresh array is first touched by the threads that fill it)
constexpr long long kScratchKeepFrames = 4000000;
struct SetScratch {
    RawVector<FrameMeta> meta;
    RawVector<FlatRef> flatRef;
    RawVector<DirectJob> directJobs;
    RawVector<FrameFacts> facts;
};
static SetScratch& set_scratch()
{
    static thread_local SetScratch scratch;
    return scratch;
}

// One set call: what its steps (batch_set) hand each other.  Everything is built here and committed to the Batch only after the
// uploads succeeded: a call that fails validation leaves the previous batch in place, one that fails while uploading leaves an
// empty batch.  The members are destroyed last to first: the staging thread is joined and the copy stream drained before anything
// they may read goes away, the scratch is released last.
struct SetCall {
    Batch* const b;
    const SetInput& in;
    const long long nL, nU;
    const long long* const listStart;
    const bool byRecords, byDevice;
    long long nF = 0;
    const std::chrono::steady_clock::time_point tSet = std::chrono::steady_clock::now();

    SetScratch& scratch = set_scratch();      // (a reference: the worker threads must write the CALLER's scratch, not their own thread_local one)
    struct ScratchRelease {
        SetScratch& s;
        long long nF = 0;
        ~ScratchRelease()
        {
            if (nF > kScratchKeepFrames) {
                RawVector<FrameMeta>().swap(s.meta); RawVector<FlatRef>().swap(s.flatRef); RawVector<FrameFacts>().swap(s.facts);
                RawVector<DirectJob>().swap(s.directJobs);
            }
        }
    } scratchRelease{scratch};
    // labels: unitFirst[] (klatt_align.h) and the units per list
    std::vector<uint32_t> unitFirst, listUnits;
    // the frames on their way
    bool framesPinned = false, earlyStarted = false;
    int earlyRc = 0;
    std::string earlyErr;
    // while a DMA reads the caller's arrays no exit may leave it running: every return passes this guard
    struct CopyGuard { Batch* b; bool armed = false; ~CopyGuard() { if (armed) (void)hipStreamSynchronize(b->copyStream); } } copyGuard{b};
    std::thread early;
    struct JoinEarly { std::thread& t; ~JoinEarly() { if (t.joinable()) t.join(); } } joinEarly{early};
    // what the planning knows of every frame
    const FrameFacts* facts = nullptr;
    bool factsOnDevice = false;
    // the plan
    ListTable lists;
    RouteOptions route;
    std::vector<uint32_t> lens;                  // per utterance: its length
    std::vector<long long> outStart, denseStart; // where its PCM goes in the pool; the utterances back to back: what speechPlayer_batch_readAll hands out
    long long total = 0, pool = 0, spoken = 0;
    TrackPlan plan;
    std::vector<uint32_t> directFirst;
    long long nDirectUtt = 0;
    bool directAligned = false;                  // route_direct's verdict; false when the call forms no direct group (Batch::directAligned)
    std::vector<UttDesc> utt;
    std::vector<uint32_t> present2;      // per utterance: its list's second word of present terms (UTT2_*)
    std::vector<long long> uttFrameStart;
    std::vector<uint32_t> uttFrames, uttList, uttSeed;
    LanePacking lanes;
    // Frames the planner recognised by their HASH are compared with the frame that first carried it, where the frames are (records
    // need none of this: a shape number IS the values).  The verdict comes back with the upload's last synchronisation.
    bool verify = false;
    unsigned long long mismatchAt = ~0ull;

    SetCall(Batch* b_, const SetInput& in_)
        : b(b_), in(in_), nL(in_.nLists), nU(in_.nUtt), listStart(in_.listStart), byRecords(in_.records != nullptr), byDevice(in_.deviceFrames != nullptr) {}
    long long list_of(long long u) const { return in.listOf ? (long long)in.listOf[u] : u; }
    void lap(const char* what) const      // SPEECHPLAYER_SET_TRACE: where the call's time goes, on stderr
    {
        static const bool setTrace = getenv("SPEECHPLAYER_SET_TRACE") != nullptr;
        if (setTrace) fprintf(stderr, "[speechPlayer/set] %s: %.1f ms since the start\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tSet).count());
    }
};

// 1. The index arrays before anything reads through them; records, labels (unitFirst[], listUnits from them).
static int set_validate(SetCall& c)
{
    const SetInput& in = c.in;
    const long long nL = c.nL, nU = c.nU;
    const long long* const listStart = c.listStart;
    if (listStart[0] != 0) { set_error("set: frameStart[0] must be 0"); return -1; }
    for (long long l = 0; l < nL; ++l)
        if (listStart[l + 1] < listStart[l]) { set_error("set: frameStart not monotone at %lld", l); return -1; }
    const long long nF = c.nF = listStart[nL];
    if (nF > 0 && !c.byRecords && ((!in.frames && !c.byDevice) || !in.minDur || !in.fadeDur)) { set_error("set: bad frame arrays"); return -1; }
    if (in.listOf) {
        FirstBad bad;
        parallel_ranges(nU, 1 << 16, [&](long long a, long long e) {
            for (long long u = a; u < e; ++u) if ((long long)in.listOf[u] >= nL) bad.mark(u);
        });
        if (bad.get() >= 0) { set_error("set: listOf[%lld] is not a list", bad.get()); return -1; }
    }
    if (c.byRecords) {
        FirstBad bad;
        parallel_ranges(nF, 1 << 16, [&](long long a, long long e) {
            for (long long k = a; k < e; ++k)
                if (in.records[k].shape != SPEECHPLAYER_RECORD_SILENCE && (long long)in.records[k].shape >= in.nShapes) bad.mark(k);
        });
        if (bad.get() >= 0) { set_error("setRecords: record %lld names shape %u of %lld", bad.get(), in.records[bad.get()].shape, in.nShapes); return -1; }
    }
    // labels: the units of a list count from 0 and rise by at most one from frame to frame; unitFirst[] (klatt_align.h) from them
    if (in.labels) {
        if (nF >= 0xFFFFFFFFll) { set_error("setRecordsLabelled: too many frames"); return -1; }
        c.unitFirst.resize((size_t)(nF + nL)); c.listUnits.assign((size_t)nL, 0);
        FirstBad bad;
        parallel_ranges(nL, 256, [&](long long la, long long le) {
            for (long long l = la; l < le; ++l) {
                uint32_t* uf = c.unitFirst.data() + listStart[l] + l;
                int units = 0;
                for (long long k = listStart[l]; k < listStart[l + 1]; ++k) {
                    const int u = in.labels[k].unit;
                    if (in.labels[k].phoneme < 0 || (u != units && !(units > 0 && u == units - 1))) { bad.mark(k); break; }
                    if (u == units) uf[units++] = (uint32_t)(k - listStart[l]);
                }
                uf[units] = (uint32_t)(listStart[l + 1] - listStart[l]);
                c.listUnits[(size_t)l] = (uint32_t)units;
            }
        });
        if (bad.get() >= 0) {
            set_error("setRecordsLabelled: label %lld (phoneme %d, unit %d): the units of a list count from 0 and rise by at most one, ids are not negative",
                      bad.get(), in.labels[bad.get()].phoneme, in.labels[bad.get()].unit);
            return -1;
        }
    }
    return 0;
}

// 2. The meta word of every frame and, from the durations alone, the length of every list.
static int set_meta_words(SetCall& c)
{
    const SetInput& in = c.in;
    const long long nL = c.nL, nF = c.nF;
    const long long* const listStart = c.listStart;
    c.scratchRelease.nF = nF;
    RawVector<FrameMeta>& meta = c.scratch.meta;
    meta.resize((size_t)nF);
    parallel_ranges(nF, 1 << 16, [&](long long a, long long e) {
        if (c.byRecords)
            for (long long k = a; k < e; ++k) {
                const speechPlayer_frameRecord_t& r = in.records[k];
                meta[k].minSamples = r.minFrameDuration;
                meta[k].fadeSamples = std::max(r.fadeDuration, 1u);      // reference src/speechPlayer.cpp:36
                meta[k].userIndex = r.userIndex;
                meta[k].flags = r.shape == SPEECHPLAYER_RECORD_SILENCE ? FRAME_NULL : 0u;
            }
        else
            for (long long k = a; k < e; ++k) {
                meta[k].minSamples = in.minDur[k];
                meta[k].fadeSamples = std::max(in.fadeDur[k], 1u);       // reference src/speechPlayer.cpp:36
                meta[k].userIndex = in.userIndex ? in.userIndex[k] : -1;
                meta[k].flags = (in.isNull && in.isNull[k]) ? FRAME_NULL : 0u;
            }
    });
    c.lists.lens.assign((size_t)nL, 0);
    FirstBad tooLong;
    parallel_ranges(nL, 4096, [&](long long la, long long le) {
        for (long long l = la; l < le; ++l)
            if (!list_length(meta.data() + listStart[l], listStart[l + 1] - listStart[l], c.lists.lens[(size_t)l])) tooLong.mark(l);
    });
    if (tooLong.get() >= 0) { set_error("utterance (frame list %lld) too long (4294967295 samples or more)", tooLong.get()); return -1; }
    return 0;
}

// 3. From here on nothing but an allocation or a copy can fail (which leaves an empty batch).  The frames -- by far the largest upload
// of a batch of full frames, 0.6 GB for BASELINE configs[2] -- start on their way now: on a thread of their own from pageable memory
// (such a copy keeps its caller until it is done), as one asynchronous DMA from page-locked memory (speechPlayer_hostAlloc); records
// travel the same way (32 bytes per frame) with their shape table, and klatt_expand_frames builds frames and meta words behind them.
static int set_start_frames(SetCall& c)
{
    Batch* const b = c.b;
    const SetInput& in = c.in;
    const long long nL = c.nL, nF = c.nF;
    // the track exports in flight read the frames, meta words and list table this call replaces
    c.framesPinned = !c.byRecords && nF > 0 && is_pinned(in.frames);
    {
        const bool grows = (size_t)nF * kNumParams > b->dFrames.cap || (size_t)nF > b->dMeta.cap || (size_t)nL + 1 > b->dListStart.cap ||
                           (in.labels && ((size_t)nF > b->dLabels.cap || (size_t)(nF + nL) > b->dUnitFirst.cap));
        const bool unordered = !c.byRecords && !c.byDevice && !c.framesPinned;      // pageable frames: copied by a thread of their own, or staged by the runtime
        if (settle_track_exports(b, grows || unordered)) return -1;
    }
    if (c.byRecords) {
        if (b->dFrames.reserve(std::max<size_t>((size_t)nF * kNumParams, 1)) || b->dMeta.reserve(std::max<size_t>((size_t)nF, 1)) ||
            b->dRecords.reserve(std::max<size_t>((size_t)nF, 1)) || b->dShapeTable.reserve(std::max<size_t>((size_t)in.nShapes * kNumParams, 1))) { batch_clear(b); return -1; }
        batch_clear(b);      // the batch on the device is the old frames with the new ones over them from now on: it no longer exists
        c.copyGuard.armed = true;
        if (in.nShapes) HIP_TRY(hipMemcpyAsync(b->dShapeTable.ptr, in.shapes, (size_t)in.nShapes * sizeof(speechPlayer_frame_t), hipMemcpyHostToDevice, b->copyStream));
        if (nF) {
            HIP_TRY(hipMemcpyAsync(b->dRecords.ptr, in.records, (size_t)nF * sizeof(FrameRecord), hipMemcpyHostToDevice, b->copyStream));
            const unsigned grid = (unsigned)std::min<long long>((nF + 63) / 64, 8192);      // tiles of 64 frames
            hipLaunchKernelGGL(klatt_expand_frames, dim3(grid), dim3(256), 0, b->copyStream, b->dRecords.ptr, b->dShapeTable.ptr, b->dFrames.ptr, b->dMeta.ptr, nF);
            HIP_TRY(hipGetLastError());
        }
        c.earlyStarted = true;
    } else if (c.byDevice && nF > 0) {
        // frames in device memory: copied device to device on the copy stream, behind what the caller's stream has queued so far
        if (in.readyStream) {
            HIP_TRY(hipEventRecord(b->inputReady, in.readyStream));
            HIP_TRY(hipStreamWaitEvent(b->copyStream, b->inputReady, 0));
        }
        if (b->dFrames.reserve((size_t)nF * kNumParams)) { batch_clear(b); return -1; }
        batch_clear(b);
        c.copyGuard.armed = true;
        HIP_TRY(hipMemcpyAsync(b->dFrames.ptr, in.deviceFrames, (size_t)nF * kNumParams * sizeof(double), hipMemcpyDeviceToDevice, b->copyStream));
        c.earlyStarted = true;
    } else if (nF > 0 && (c.framesPinned || (size_t)nF * kNumParams * sizeof(double) >= (32u << 20))) {
        if (b->dFrames.reserve((size_t)nF * kNumParams)) { batch_clear(b); return -1; }
        batch_clear(b);
        if (c.framesPinned) {
            c.copyGuard.armed = true;
            HIP_TRY(hipMemcpyAsync(b->dFrames.ptr, in.frames, (size_t)nF * kNumParams * sizeof(double), hipMemcpyHostToDevice, b->copyStream));
            c.earlyStarted = true;
        } else
        try {
            c.early = std::thread([&c, frames = in.frames, nF, dev = b->device, dst = b->dFrames.ptr]() {
                hipError_t e = hipSetDevice(dev);
                if (e == hipSuccess) e = hipMemcpy(dst, frames, (size_t)nF * kNumParams * sizeof(double), hipMemcpyHostToDevice);
                if (e != hipSuccess) { c.earlyRc = -1; c.earlyErr = hipGetErrorString(e); }
            });
            c.earlyStarted = true;
        } catch (const std::system_error&) {}
    }
    return 0;
}

// 4. What the planning needs to know of every frame (klatt_plan.h: a word of flags, and something that stands for its 45 shape values),
// in ONE pass.  Records: the flags of their shape (evaluated once per row of the table) and of their pitches; the shape's number
// stands for the values, exactly.  Frames on their way to the device as a DMA (page-locked memory) are looked at THERE, behind the
// copy on the same stream, and 24 bytes per frame come back: the host never reads them (set_plan waits for them, as late as it can).
// Pageable frames are read here, by the host's threads, while the staging thread copies them.
static int set_frame_facts(SetCall& c)
{
    Batch* const b = c.b;
    const SetInput& in = c.in;
    const long long nF = c.nF;
    const double maxBwDirect = 690.0 * b->sampleRate / M_PI, maxFDirect = 9900.0 * b->sampleRate / (2.0 * M_PI);
    c.factsOnDevice = (c.framesPinned || c.byDevice) && c.earlyStarted;
    RawVector<FrameFacts>& fv = c.scratch.facts;
    if (c.byRecords) {
        std::vector<uint32_t> shapeFl((size_t)in.nShapes), shapeP2((size_t)in.nShapes);
        for (long long s = 0; s < in.nShapes; ++s) {
            shapeFl[(size_t)s] = shape_flags(reinterpret_cast<const double*>(in.shapes + s), maxFDirect, maxBwDirect);
            shapeP2[(size_t)s] = shape_present2(reinterpret_cast<const double*>(in.shapes + s));
        }
        fv.resize((size_t)nF);
        parallel_ranges(nF, 1 << 15, [&](long long a, long long e) {
            for (long long k = a; k < e; ++k) {
                const speechPlayer_frameRecord_t& r = in.records[k];
                FrameFacts f;
                f.h0 = r.shape; f.h1 = ~0ull;
                f.flags = r.shape == SPEECHPLAYER_RECORD_SILENCE ? 0u : (shapeFl[r.shape] | pitch_flags(r.voicePitch, r.endVoicePitch));
                // (a silence record sets no bit in either word, where frame_facts on its all-zero frame would set several: it is a NULL frame, which classify_list skips)
                f.present2 = r.shape == SPEECHPLAYER_RECORD_SILENCE ? 0u : present2_of(f.flags, shapeP2[r.shape]);
                fv[k] = f;
            }
        });
        c.facts = fv.data();
    } else if (c.factsOnDevice) {
        if (b->dFacts.reserve((size_t)nF) || b->hFacts.ensure((size_t)nF * sizeof(FrameFacts))) return -1;
        const unsigned grid = (unsigned)std::min<long long>((nF + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(klatt_frame_facts, dim3(grid), dim3(256), 0, b->copyStream, b->dFrames.ptr, b->dFacts.ptr, nF, maxFDirect, maxBwDirect);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(b->hFacts.ptr, b->dFacts.ptr, (size_t)nF * sizeof(FrameFacts), hipMemcpyDeviceToHost, b->copyStream));
        c.facts = static_cast<const FrameFacts*>(b->hFacts.ptr);
    } else if (nF > 0) {
        fv.resize((size_t)nF);
        parallel_ranges(nF, 1 << 13, [&](long long a, long long e) {
            for (long long k = a; k < e; ++k) fv[k] = frame_facts(reinterpret_cast<const double*>(in.frames + k), maxFDirect, maxBwDirect);
        });
        c.facts = fv.data();
    }
    return 0;
}

// 5. The plan (klatt_batchplan.h): per utterance its length and where its PCM goes; per list its timing, its class and the kernels
// its utterances go to, with plan_tracks in the middle.
static int set_plan(SetCall& c)
{
    Batch* const b = c.b;
    const SetInput& in = c.in;
    const long long nL = c.nL, nU = c.nU, nF = c.nF;
    const long long* const listStart = c.listStart;
    const FrameMeta* const meta = c.scratch.meta.data();
    ListTable& lists = c.lists;
    c.lens.assign((size_t)nU, 0);
    c.outStart.assign((size_t)nU + 1, 0);
    c.denseStart.resize((size_t)nU + 1);
    for (long long u = 0; u < nU; ++u) {
        const long long l = c.list_of(u);
        c.lens[u] = lists.lens[l];
        c.outStart[u] = c.pool;
        c.denseStart[u] = c.total;
        c.total += (long long)c.lens[u];
        c.pool += ((long long)c.lens[u] + kTile - 1) / kTile * kTile;
        c.spoken += listStart[l + 1] - listStart[l];
    }
    c.outStart[nU] = c.pool;
    c.denseStart[nU] = c.total;
    // how many utterances speak each list
    lists.weight.assign((size_t)nL, in.listOf ? 0u : 1u);
    if (in.listOf) for (long long u = 0; u < nU; ++u) ++lists.weight[in.listOf[u]];
    c.lap("meta, lengths, frame facts started");
    lists.timing.resize((size_t)nL);
    parallel_ranges(nL, 4096, [&](long long la, long long le) {
        for (long long l = la; l < le; ++l) lists.timing[l] = list_timing(meta + listStart[l], listStart[l + 1] - listStart[l]);
    });
    // the facts are back (device path), only now: the timing hashes above needed none of them
    if (c.factsOnDevice) HIP_TRY(hipStreamSynchronize(b->copyStream));
    const FrameFacts* const facts = c.facts;
    lists.shape.assign((size_t)nL, 0);
    lists.flags.assign((size_t)nL, 0);
    lists.present2.assign((size_t)nL, 0);
    parallel_ranges(nL, 4096, [&](long long la, long long le) {
        for (long long l = la; l < le; ++l)
            classify_list(meta + listStart[l], facts + listStart[l], listStart[l + 1] - listStart[l], lists.flags[l], lists.shape[l], lists.present2[l]);
    });
    c.lap("classification");
    RouteOptions& route = c.route;
    route.tracks = b->tracks; route.direct = b->direct; route.layout = b->layout;
    route.fast = b->mode == MODE_FAST; route.sortByLength = b->sortByLength != 0; route.noTracks = in.noTracks;
    route.cus = b->cus; route.nFrames = nF;
    const Rerouted rerouted = reroute_lonely_quiet(lists, route);
    c.lap("timing hashes, quiet runs");
    const std::vector<unsigned char> eligible = eligible_lists(lists, route);
    c.lap("eligibility");
    TrackPlan& plan = c.plan;
    FrameSource source{in.frames, in.records, in.shapes};
    RawVector<uint32_t> rowOf;
    std::vector<long long> shapeRep;
    std::vector<double> shapeRows;
    const bool wantTracks = route.want_tracks() && nF > 0;
    const HashMask hashMask = plan_hash_mask();
    if (wantTracks && c.byDevice) {
        if (device_shape_table(b, nL, listStart, meta, facts, eligible.data(), hashMask, rowOf, shapeRep, shapeRows)) return -1;
        source.shapes = reinterpret_cast<const speechPlayer_frame_t*>(shapeRows.data());
        source.rowOf = rowOf.data();
        c.lap("shape table");
    }
    if (wantTracks) {
        plan_tracks(nL, listStart, source, facts, meta, eligible.data(), track_budget_entries(b->trackBudgetMB), hashMask, plan);
        if (source.rowOf && !plan.rep.empty()) {
            // every frame the planner took values for stands for the table's row: each is compared with the row's frame (klatt_verify_shared)
            parallel_ranges(nL, 4096, [&](long long la, long long le) {
                for (long long l = la; l < le; ++l) {
                    if (!eligible[l]) continue;
                    for (long long k = listStart[l]; k < listStart[l + 1]; ++k) {
                        if (meta[k].flags & FRAME_NULL) continue;
                        const long long r = shapeRep[rowOf[k]];
                        plan.rep[k] = r == k ? 0xFFFFFFFFu : (uint32_t)r;
                    }
                }
            });
        }
        c.lap("tracks planned");
        if (tracks_pay(lists, eligible.data(), plan.tracked.data(), plan.entries * sizeof(double2), route)) mark_tracked(lists, plan.tracked.data(), plan.kinds.data());
        else { plan.jobs.clear(); plan.entries = 0; plan.tracked.assign((size_t)nL, 0); }
    }
    if (route.want_direct()) c.directAligned = route_direct(lists, eligible.data(), route);
    restore_rerouted(lists, rerouted);
    return 0;
}

// 6. The direct lists' fades: per frame where its fade starts from and ends on (reference src/frame.cpp:55-72: silence keeps
// the previous request's values with the gain gated off; the first frame after silence starts from its own values with the gain
// gated off; any other frame fades from the previous request's values) -- klatt_seeds reads the values themselves on the device.
// And what a flat stage needs of a frame when its fade starts (FlatRef), where there are tracks.
static void set_direct_jobs_and_refs(SetCall& c)
{
    const long long nL = c.nL, nU = c.nU, nF = c.nF;
    const long long* const listStart = c.listStart;
    const RawVector<FrameMeta>& meta = c.scratch.meta;
    const TrackPlan& plan = c.plan;
    RawVector<DirectJob>& directJobs = c.scratch.directJobs;
    directJobs.clear();
    if (c.route.want_direct()) {
        std::vector<uint32_t> directFirstL((size_t)nL, 0u);
        for (long long l = 0; l < nL; ++l) {
            if (!(c.lists.flags[l] & UTT_DIRECT)) continue;
            c.nDirectUtt += c.lists.weight[l];
            directFirstL[l] = (uint32_t)directJobs.size();
            walk_fade_ends(listStart[l], listStart[l + 1], meta.data(), directJobs);
        }
        c.directFirst.resize((size_t)nU);
        parallel_ranges(nU, 1 << 16, [&](long long a, long long e) { for (long long u = a; u < e; ++u) c.directFirst[u] = directFirstL[c.list_of(u)]; });
    }
    RawVector<FlatRef>& flatRef = c.scratch.flatRef;
    if (!plan.jobs.empty()) {
        flatRef.resize((size_t)nF);
        parallel_ranges(nF, 1 << 16, [&](long long ka, long long ke) {
        for (long long k = ka; k < ke; ++k) {
            const unsigned long long m = meta[k].minSamples, f = meta[k].fadeSamples;
            flatRef[k] = FlatRef{(uint32_t)plan.ref[k].off, plan.ref[k].mask, meta[k].fadeSamples, (uint32_t)std::min<unsigned long long>(std::max(m, f + 1) + 1, 0xFFFFFFFFull)};
        }
        });
    }
    c.lap("direct jobs, flat / source references");
}

// 7. The utterances, each with its list's frames, flags and length, in their lanes (klatt_batchplan.h, pack_lanes).
static void set_lanes(SetCall& c)
{
    const SetInput& in = c.in;
    const long long nU = c.nU;
    const long long* const listStart = c.listStart;
    c.utt.resize((size_t)nU); c.present2.resize((size_t)nU); c.uttFrameStart.resize((size_t)nU); c.uttFrames.resize((size_t)nU); c.uttList.resize((size_t)nU); c.uttSeed.resize((size_t)nU);
    parallel_ranges(nU, 1 << 15, [&](long long a, long long e) {
        for (long long u = a; u < e; ++u) {
            const long long l = c.list_of(u);
            UttDesc d;
            d.frameStart = listStart[l];
            d.outStart = c.outStart[u];
            d.nFrames = (uint32_t)(listStart[l + 1] - listStart[l]);
            d.seed = in.seeds ? in.seeds[u] : (uint32_t)u;
            d.flags = c.lists.flags[l];
            d.length = c.lists.lens[l];
            c.utt[u] = d;
            c.present2[u] = c.lists.present2[l];
            c.uttFrameStart[u] = d.frameStart; c.uttFrames[u] = d.nFrames; c.uttList[u] = (uint32_t)l; c.uttSeed[u] = d.seed;
        }
    });
    std::vector<unsigned long long> timing;      // per utterance (its list's)
    if (in.listOf) { timing.resize((size_t)nU); for (long long u = 0; u < nU; ++u) timing[u] = c.lists.timing[in.listOf[u]]; }
    else timing.swap(c.lists.timing);
    c.lanes = pack_lanes(nU, [&](uint32_t u) { return c.utt[u].flags; }, c.lens.data(), timing.data(), c.b->sortByLength != 0);
    c.lap("lane packing");
}

// 8. Everything else goes up on the batch's stream, the labels on the copy stream ahead of setCopied; then the frames have arrived,
// and what is computed from them where they are: the verdict on the hashed shapes, the source references.
static int set_upload(SetCall& c)
{
    Batch* const b = c.b;
    const SetInput& in = c.in;
    const long long nL = c.nL, nU = c.nU, nF = c.nF, pool = c.pool, nSlotsAll = (long long)c.lanes.order.size();
    const long long nTrackedUtt = c.lanes.nTrackedUtt, nDirectUtt = c.nDirectUtt;
    const TrackPlan& plan = c.plan;
    const RawVector<DirectJob>& directJobs = c.scratch.directJobs;
    if ((size_t)pool > b->dPcm.cap && sync_exports(b)) return -1;      // (a new pool: the old one is freed once no export reads it)
    if (b->dFrames.reserve(std::max<size_t>((size_t)nF * kNumParams, 1)) || b->dMeta.reserve(std::max<size_t>(nF, 1)) ||
        b->dUtt.reserve(std::max<size_t>(nU, 1)) || b->dOrder.reserve(std::max<size_t>(nSlotsAll, 1)) ||
        b->dResult.reserve(std::max<size_t>(nU, 1)) || b->dPcm.reserve(std::max<size_t>(pool, 1)) || b->dListStart.reserve((size_t)nL + 1))
        return -1;
    HIP_TRY(hipMemcpyAsync(b->dListStart.ptr, c.listStart, ((size_t)nL + 1) * sizeof(long long), hipMemcpyHostToDevice, b->stream));
    if (nTrackedUtt > 0) {
        if (b->dFlatRef.reserve((size_t)nF) || b->dJobs.reserve(plan.jobs.size()) || b->dShapes.reserve(plan.shapes.size()) ||
            b->dTrack.reserve((size_t)plan.entries + kTrackPad)) return -1;
        HIP_TRY(hipMemcpyAsync(b->dShapes.ptr, plan.shapes.data(), plan.shapes.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->dFlatRef.ptr, c.scratch.flatRef.data(), (size_t)nF * sizeof(FlatRef), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->dJobs.ptr, plan.jobs.data(), plan.jobs.size() * sizeof(TrackJob), hipMemcpyHostToDevice, b->stream));
    }
    if (nTrackedUtt > 0 || nDirectUtt > 0) {
        if (b->dSourceRef.reserve((size_t)nF)) return -1;
    }
    if (nTrackedUtt > 0) {
        if (b->dPresent2.reserve((size_t)nU)) return -1;
        HIP_TRY(hipMemcpyAsync(b->dPresent2.ptr, c.present2.data(), (size_t)nU * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    }
    if (nDirectUtt > 0) {
        const size_t nD = directJobs.size();
        if (b->dDirectJobs.reserve(nD) || b->dDirectFirst.reserve((size_t)nU) || b->dDirectHdr.reserve((size_t)kDirectStages * nD) ||
            b->dDirectRec.reserve((size_t)kDirectEntries * nD)) return -1;
        HIP_TRY(hipMemcpyAsync(b->dDirectJobs.ptr, directJobs.data(), nD * sizeof(DirectJob), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->dDirectFirst.ptr, c.directFirst.data(), (size_t)nU * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    }
    if (nF) {
        if (!c.earlyStarted) HIP_TRY(hipMemcpyAsync(b->dFrames.ptr, in.frames, (size_t)nF * kNumParams * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (!c.byRecords) HIP_TRY(hipMemcpyAsync(b->dMeta.ptr, c.scratch.meta.data(), (size_t)nF * sizeof(FrameMeta), hipMemcpyHostToDevice, b->stream));
    }
    if (nU) {
        HIP_TRY(hipMemcpyAsync(b->dUtt.ptr, c.utt.data(), (size_t)nU * sizeof(UttDesc), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->dOrder.ptr, c.lanes.order.data(), (size_t)nSlotsAll * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemsetAsync(b->dResult.ptr, 0, (size_t)nU * sizeof(UttResult), b->stream));
        if (b->dDenseStart.reserve((size_t)nU + 1)) return -1;
        HIP_TRY(hipMemcpyAsync(b->dDenseStart.ptr, c.denseStart.data(), ((size_t)nU + 1) * sizeof(long long), hipMemcpyHostToDevice, b->stream));
    }
    if (c.verify) {
        if (b->dRep.reserve((size_t)nF) || b->dMismatch.reserve(1)) return -1;
        HIP_TRY(hipMemcpyAsync(b->dRep.ptr, plan.rep.data(), (size_t)nF * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemsetAsync(b->dMismatch.ptr, 0xFF, sizeof(unsigned long long), b->stream));
    }
    if (in.labels) {
        // the labels and unitFirst[] (klatt_align.h) on the copy stream, ahead of setCopied; the wait below covers the arrays they leave
        if (b->dLabels.reserve(std::max<size_t>((size_t)nF, 1)) || b->dUnitFirst.reserve(std::max<size_t>((size_t)(nF + nL), 1))) return -1;
        c.copyGuard.armed = true;
        if (nF) HIP_TRY(hipMemcpyAsync(b->dLabels.ptr, in.labels, (size_t)nF * sizeof(FrameLabel), hipMemcpyHostToDevice, b->copyStream));
        if (nF + nL) HIP_TRY(hipMemcpyAsync(b->dUnitFirst.ptr, c.unitFirst.data(), (size_t)(nF + nL) * sizeof(uint32_t), hipMemcpyHostToDevice, b->copyStream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (c.copyGuard.armed) { HIP_TRY(hipStreamSynchronize(b->copyStream)); c.copyGuard.armed = false; }
    if (c.early.joinable()) c.early.join();
    if (c.earlyRc) { set_error_code(SPEECHPLAYER_ERR_HIP); set_error("set: uploading the frames failed: %s", c.earlyErr.c_str()); return -1; }
    const unsigned grid = (unsigned)std::min<long long>((nF + 255) / 256, 1 << 16);
    if (c.verify) {
        hipLaunchKernelGGL(klatt_verify_shared, dim3(grid), dim3(256), 0, b->stream, b->dFrames.ptr, b->dRep.ptr, nF, b->dMismatch.ptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.mismatchAt, b->dMismatch.ptr, sizeof c.mismatchAt, hipMemcpyDeviceToHost, b->stream));
    }
    if (nTrackedUtt > 0 || nDirectUtt > 0) {
        // what the flat and direct source stages read at a dequeue (SourceRef: pitch, pitch increment, 1 / fade, index mark), from the
        // frames and durations now resident: 32 bytes per frame that no longer cross the link, and no third pass of the host over the frames
        hipLaunchKernelGGL(klatt_source_refs, dim3(grid), dim3(256), 0, b->stream, b->dFrames.ptr, b->dMeta.ptr, b->dSourceRef.ptr, nF);
        HIP_TRY(hipGetLastError());
    }
    if (c.verify || nTrackedUtt > 0 || nDirectUtt > 0) HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

// 10. The call has succeeded: the Batch takes what it built.
static int set_commit(SetCall& c)
{
    Batch* const b = c.b;
    const LanePacking& lanes = c.lanes;
    b->hasLabels = c.in.labels != nullptr;
    b->listUnits.swap(c.listUnits);
    b->nUtt = c.nU; b->nFrames = c.nF; b->nFramesSpoken = c.spoken; b->nLists = c.nL; b->nSlots = (long long)lanes.order.size();
    b->nNoNasalUtt = lanes.nNoNasal;
    b->nQuiet = lanes.nQuietSlots; b->nNoNasal = lanes.nNoNasalSlots;      // (slots: the groups' utterances and the replicas that complete their sparse last wavefronts)
    b->nTracked = lanes.nTrackedUtt > 0 ? lanes.nTracked : 0; b->nTrackedUtt = lanes.nTrackedUtt;
    dead_wave_counts(lanes.order.data(), lanes.nQuietSlots, b->nTracked, [&](uint32_t u) { return c.utt[u].flags; }, KLATT_DEAD_TERMS, b->planDeadWaves);
    dead2_wave_counts(lanes.order.data(), lanes.nQuietSlots, b->nTracked, [&](uint32_t u) { return c.utt[u].flags; }, [&](uint32_t u) { return c.present2[u]; },
                      KLATT_DEAD_TERMS, b->planDead2Waves);
    b->nJobs = lanes.nTrackedUtt > 0 ? (long long)c.plan.jobs.size() : 0; b->trackEntries = lanes.nTrackedUtt > 0 ? (long long)c.plan.entries : 0;
    b->nDirect = c.nDirectUtt > 0 ? lanes.nDirectSlots : 0; b->nDirectUtt = c.nDirectUtt; b->nDirectFrames = (long long)c.scratch.directJobs.size();
    b->directAligned = c.nDirectUtt > 0 && c.directAligned;
    b->totalSamples = c.total; b->poolSamples = c.pool;
    b->lens.swap(c.lens); b->outStart.swap(c.outStart); b->denseStart.swap(c.denseStart);
    b->uttFrameStart.swap(c.uttFrameStart); b->uttFrames.swap(c.uttFrames); b->uttList.swap(c.uttList); b->uttSeed.swap(c.uttSeed);
    b->timelineFresh = false; b->epochFresh = false;
    // (what this call left queued on its two streams, if anything: the track exports wait for it on the device)
    HIP_TRY(hipEventRecord(b->setDone, b->stream));
    HIP_TRY(hipEventRecord(b->setCopied, b->copyStream));
    b->results.clear();
    b->resultsFresh = false;
    b->floatFresh = false;
    b->launched = false;
    return 0;
}

// Setting a batch, behind all five entry points.  The order of events is where the call's measured time comes from: the frames
// start on their way (3) before anybody looks at them (4), the facts computed on the device are waited for only after the timing
// hashes (in 5), and the labels travel on the copy stream ahead of setCopied (8).
static int batch_set(Batch* b, const SetInput& in)
{
    if (!b || in.nLists < 0 || in.nUtt < 0 || !in.listStart) { set_error("set: bad arguments"); return -1; }
    if (in.nUtt >= 0xFFFFFFFFll || in.nLists >= 0xFFFFFFFFll) { set_error("set: too many utterances"); return -1; }
    if (!in.listOf && in.nUtt != in.nLists) { set_error("set: %lld utterances for %lld lists and no listOf", in.nUtt, in.nLists); return -1; }
    SetCall c(b, in);
    HIP_TRY(hipSetDevice(b->device));
    if (set_validate(c) || set_meta_words(c)) return -1;      // (the previous batch stays)
    if (set_start_frames(c) || set_frame_facts(c) || set_plan(c)) return -1;
    set_direct_jobs_and_refs(c);
    set_lanes(c);
    c.verify = !c.byRecords && c.lanes.nTrackedUtt > 0 && !c.plan.rep.empty();
    if (set_upload(c)) {
        // the device buffers may hold a mix of the old and the new batch now: the object becomes an empty batch
        batch_clear(b);
        return -1;
    }
    c.lap("uploads");
    if (c.verify && c.mismatchAt != ~0ull) {
        // 9. two frames with one hash and different values: the plan built on their equality is void.  The batch is planned again
        // without tracks (nothing else rests on the hash) and the caller is told -- the call succeeds, the message stays.
        const unsigned long long k = c.mismatchAt;
        if (c.early.joinable()) c.early.join();
        SetInput again = in;
        again.noTracks = true;
        const uint32_t first = c.plan.rep[(size_t)k];
        const int rc = batch_set(b, again);
        if (rc == 0) {
            set_error("set: frames %llu and %u carry one 128-bit shape hash and different values; the batch runs without tracks", k, first);
            set_error_code(SPEECHPLAYER_OK);
        }
        return rc;
    }
    return set_commit(c);
}

long long speechPlayer_batch_frames(speechPlayer_batch_t batch, long long u, speechPlayer_frame_t* frames, unsigned int* minFrameDuration,
                                    unsigned int* fadeDuration, int* userIndex, unsigned char* isNull, long long capacity)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt) { set_error("batch_frames: no such utterance"); return -1; }
    HIP_TRY(hipSetDevice(b->device));
    const long long n = b->uttFrames[(size_t)u], k0 = b->uttFrameStart[(size_t)u];
    if (n > capacity || n == 0) return n;
    if (frames) HIP_TRY(hipMemcpy(frames, b->dFrames.ptr + k0 * kNumParams, (size_t)n * sizeof(speechPlayer_frame_t), hipMemcpyDeviceToHost));
    if (minFrameDuration || fadeDuration || userIndex || isNull) {
        std::vector<FrameMeta> m((size_t)n);
        HIP_TRY(hipMemcpy(m.data(), b->dMeta.ptr + k0, (size_t)n * sizeof(FrameMeta), hipMemcpyDeviceToHost));
        for (long long k = 0; k < n; ++k) {
            if (minFrameDuration) minFrameDuration[k] = m[(size_t)k].minSamples;
            if (fadeDuration) fadeDuration[k] = m[(size_t)k].fadeSamples;
            if (userIndex) userIndex[k] = m[(size_t)k].userIndex;
            if (isNull) isNull[k] = (m[(size_t)k].flags & FRAME_NULL) ? 1 : 0;
        }
    }
    return n;
}

long long speechPlayer_batch_utteranceSamples(speechPlayer_batch_t batch, long long u)
{
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt) return -1;
    return b->lens[u];
}
long long speechPlayer_batch_lengths(speechPlayer_batch_t batch, long long* lengths, long long capacity)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) { set_error("batch_lengths: no batch"); return -1; }
    if (lengths && b->nUtt <= capacity)
        for (long long u = 0; u < b->nUtt; ++u) lengths[u] = b->lens[(size_t)u];
    return b->nUtt;
}
long long speechPlayer_batch_totalSamples(speechPlayer_batch_t batch) { return batch ? static_cast<Batch*>(batch)->totalSamples : -1; }
long long speechPlayer_batch_totalFrames(speechPlayer_batch_t batch) { return batch ? static_cast<Batch*>(batch)->nFramesSpoken : -1; }
int speechPlayer_batch_sampleRate(speechPlayer_batch_t batch) { return batch ? static_cast<Batch*>(batch)->sampleRate : -1; }

int speechPlayer_batch_synthesize(speechPlayer_batch_t batch)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) return -1;
    HIP_TRY(hipSetDevice(b->device));
    return batch_launch(b);
}

int speechPlayer_batch_wait(speechPlayer_batch_t batch)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) return -1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

static int fetch_results(Batch* b)
{
    if (b->resultsFresh) return 0;
    b->results.resize((size_t)b->nUtt);
    if (b->nUtt) HIP_TRY(hipMemcpy(b->results.data(), b->dResult.ptr, (size_t)b->nUtt * sizeof(UttResult), hipMemcpyDeviceToHost));
    b->resultsFresh = true;
    return 0;
}

long long speechPlayer_batch_read(speechPlayer_batch_t batch, long long u, sample* sampleBuf, long long capacity)
{
    begin_call();
    if (refuse_timing_only("speechPlayer_batch_read")) return -1;
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt || !sampleBuf) return -1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (fetch_results(b)) return -1;
    long long n = std::min<long long>(b->results[u].produced, capacity);
    if (n > 0) HIP_TRY(hipMemcpy(sampleBuf, b->dPcm.ptr + b->outStart[u], (size_t)n * sizeof(int16_t), hipMemcpyDeviceToHost));
    return n;
}

// The utterances back to back in HBM (pcm_compact), queued on the batch's stream behind the synthesis; `denseReady` marks the end.
static int dense_prepare(Batch* b)
{
    const long long total = b->totalSamples;
    if (b->copyPending) { HIP_TRY(hipEventSynchronize(b->copyDone)); b->copyPending = false; }      // the previous copy still reads dDense (before it may be re-allocated)
    if (b->dDense.reserve((size_t)((total + 7) / 8 * 8 + 8))) return -1;
    const long long n8 = (total + 7) / 8;
    if (n8 > 0) {
        const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(pcm_compact, dim3(grid), dim3(256), 0, b->stream, b->dPcm.ptr, b->dDense.ptr, b->dUtt.ptr, b->dDenseStart.ptr, b->nUtt, total);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(b->denseReady, b->stream));
    return 0;
}

// Before round 5 (and still, for a batch that has not been synthesised to the end: produced != length somewhere): the padded pool comes
// over in 16 MB pieces through two pinned buffers and one host thread compacts them into the caller's buffer.
static long long read_all_padded(Batch* b, sample* sampleBuf, long long capacity, long long* outStart)
{
    std::vector<long long> dstStart((size_t)b->nUtt + 1);
    long long pos = 0;
    for (long long u = 0; u < b->nUtt; ++u) { dstStart[u] = pos; pos += b->results[u].produced; }
    dstStart[b->nUtt] = pos;
    if (pos > capacity) { set_error("readAll: capacity %lld too small for %lld samples", capacity, pos); return -1; }
    if (outStart) memcpy(outStart, dstStart.data(), sizeof(long long) * ((size_t)b->nUtt + 1));
    constexpr long long kPiece = 8ll << 20;   // samples
    if (b->bounce.ensure((size_t)kPiece * sizeof(int16_t))) return -1;
    const long long nPieces = (b->poolSamples + kPiece - 1) / kPiece;
    auto issue = [&](long long k) -> int {
        const long long off = k * kPiece, n = std::min(kPiece, b->poolSamples - off);
        HIP_TRY(hipMemcpyAsync(b->bounce.buf[k & 1], b->dPcm.ptr + off, (size_t)n * sizeof(int16_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipEventRecord(b->bounce.ev[k & 1], b->stream));
        return 0;
    };
    if (nPieces > 0 && issue(0)) return -1;
    int16_t* const dst = reinterpret_cast<int16_t*>(sampleBuf);
    long long u = 0;
    for (long long k = 0; k < nPieces; ++k) {
        if (k + 1 < nPieces && issue(k + 1)) return -1;
        HIP_TRY(hipEventSynchronize(b->bounce.ev[k & 1]));
        const long long c0 = k * kPiece, c1 = std::min(c0 + kPiece, b->poolSamples);
        const int16_t* const src = static_cast<const int16_t*>(b->bounce.buf[k & 1]);
        while (u < b->nUtt) {
            const long long s0 = b->outStart[u], e0 = s0 + b->results[u].produced;
            if (s0 >= c1) break;
            const long long lo = std::max(s0, c0), hi = std::min(e0, c1);
            if (hi > lo) memcpy(dst + dstStart[u] + (lo - s0), src + (lo - c0), (size_t)(hi - lo) * sizeof(int16_t));
            if (e0 > c1) break;       // continues in the next piece
            ++u;
        }
    }
    return pos;
}

long long speechPlayer_batch_readAll(speechPlayer_batch_t batch, sample* sampleBuf, long long capacity, long long* outStart)
{
    begin_call();
    if (refuse_timing_only("speechPlayer_batch_readAll")) return -1;
    Batch* b = static_cast<Batch*>(batch);
    if (!b || !sampleBuf) return -1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (fetch_results(b)) return -1;
    bool whole = true;      // every utterance synthesised to its end (a batch launch always does; a batch never launched has produced nothing)
    for (long long u = 0; u < b->nUtt && whole; ++u) whole = b->results[u].produced == b->lens[u];
    if (!whole) return read_all_padded(b, sampleBuf, capacity, outStart);
    const long long total = b->totalSamples;
    if (total > capacity) { set_error("readAll: capacity %lld too small for %lld samples", capacity, total); return -1; }
    if (outStart) memcpy(outStart, b->denseStart.data(), sizeof(long long) * ((size_t)b->nUtt + 1));
    if (total == 0) return 0;
    // dense order on the device first; then the bytes cross the link as they will lie in the caller's buffer
    if (dense_prepare(b)) return -1;
    HIP_TRY(hipStreamWaitEvent(b->copyStream, b->denseReady, 0));
    if (is_pinned(sampleBuf)) {
        HIP_TRY(hipMemcpyAsync(sampleBuf, b->dDense.ptr, (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost, b->copyStream));
        HIP_TRY(hipStreamSynchronize(b->copyStream));
        return total;
    }
    // pageable destination: 32 MB pieces through two pinned buffers, piece k + 1 in flight while piece k is copied out (a plain memcpy now)
    constexpr long long kPiece = 16ll << 20;   // samples
    if (b->bounce.ensure((size_t)kPiece * sizeof(int16_t))) return -1;
    const long long nPieces = (total + kPiece - 1) / kPiece;
    auto issue = [&](long long k) -> int {
        const long long off = k * kPiece, n = std::min(kPiece, total - off);
        HIP_TRY(hipMemcpyAsync(b->bounce.buf[k & 1], b->dDense.ptr + off, (size_t)n * sizeof(int16_t), hipMemcpyDeviceToHost, b->copyStream));
        HIP_TRY(hipEventRecord(b->bounce.ev[k & 1], b->copyStream));
        return 0;
    };
    if (issue(0)) return -1;
    int16_t* const dst = reinterpret_cast<int16_t*>(sampleBuf);
    for (long long k = 0; k < nPieces; ++k) {
        HIP_TRY(hipEventSynchronize(b->bounce.ev[k & 1]));
        const long long off = k * kPiece, n = std::min(kPiece, total - off);
        // (the other buffer's copy is issued only after this one has been emptied two pieces ago: buffers alternate)
        if (k + 1 < nPieces && issue(k + 1)) return -1;
        const int16_t* const src = static_cast<const int16_t*>(b->bounce.buf[k & 1]);
        parallel_ranges(n, 1 << 21, [&](long long a, long long e) { memcpy(dst + off + a, src + a, (size_t)(e - a) * sizeof(int16_t)); });
    }
    return total;
}

// readAll without waiting: the compaction and ONE copy into page-locked memory (speechPlayer_hostAlloc, or registered by the caller) are
// queued behind the synthesis and the call returns; the copy runs on a stream of its own, beside whatever is launched next (another
// batch's synthesis, this batch's next launch: the pool is free again as soon as the compaction has run).  speechPlayer_batch_readWait
// waits for it.  Returns the number of samples that will arrive, -1 when the buffer is not page-locked or too small.
long long speechPlayer_batch_readAllAsync(speechPlayer_batch_t batch, sample* sampleBuf, long long capacity, long long* outStart)
{
    begin_call();
    if (refuse_timing_only("speechPlayer_batch_readAllAsync")) return -1;
    Batch* b = static_cast<Batch*>(batch);
    if (!b || !sampleBuf) return -1;
    HIP_TRY(hipSetDevice(b->device));
    if (!is_pinned(sampleBuf)) { set_error("readAllAsync: the buffer is not page-locked (speechPlayer_hostAlloc)"); return -1; }
    // (readAll checks what every utterance produced and falls back to the padded copy; this call cannot wait for that -- it needs a launch
    // queued since the batch was set: a batch launch always synthesises every utterance to its end.  ADVICE r5)
    if (!b->launched && b->nUtt > 0) { set_error("readAllAsync: the batch has not been synthesised since it was set"); return -1; }
    const long long total = b->totalSamples;
    if (total > capacity) { set_error("readAllAsync: capacity %lld too small for %lld samples", capacity, total); return -1; }
    if (outStart) memcpy(outStart, b->denseStart.data(), sizeof(long long) * ((size_t)b->nUtt + 1));
    if (total == 0) return 0;
    if (dense_prepare(b)) return -1;
    HIP_TRY(hipStreamWaitEvent(b->copyStream, b->denseReady, 0));
    HIP_TRY(hipMemcpyAsync(sampleBuf, b->dDense.ptr, (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost, b->copyStream));
    HIP_TRY(hipEventRecord(b->copyDone, b->copyStream));
    b->copyPending = true;
    return total;
}

int speechPlayer_batch_readWait(speechPlayer_batch_t batch)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) return -1;
    HIP_TRY(hipSetDevice(b->device));
    if (b->copyPending) { HIP_TRY(hipEventSynchronize(b->copyDone)); b->copyPending = false; }
    return 0;
}

// Page-locked host memory for the two large transfers of a batch -- frames in (speechPlayer_batch_setUtterances), PCM out
// (speechPlayer_batch_readAll / readAllAsync): a buffer from here travels as one DMA at the link's rate.  NULL when it cannot be had.
void* speechPlayer_hostAlloc(long long bytes)
{
    begin_call();
    if (bytes <= 0) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        set_error_code(SPEECHPLAYER_ERR_HIP);
        set_error("hostAlloc: cannot page-lock %lld bytes", bytes);
        return nullptr;
    }
    return p;
}
void speechPlayer_hostFree(void* p)
{
    if (p) (void)hipHostFree(p);
}

long long speechPlayer_batch_readFloat(speechPlayer_batch_t batch, long long u, float* sampleBuf, long long capacity)
{
    begin_call();
    if (refuse_timing_only("speechPlayer_batch_readFloat")) return -1;
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt || !sampleBuf) return -1;
    HIP_TRY(hipSetDevice(b->device));
    if (!b->floatFresh) {
        if (b->dFloat.reserve(std::max<size_t>(b->poolSamples, 8))) return -1;
        const long long n8 = b->poolSamples / 8;     // the pool is a multiple of 32 samples
        if (n8 > 0) {
            const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 2048);
            hipLaunchKernelGGL(pcm_to_float, dim3(grid), dim3(256), 0, b->stream, b->dPcm.ptr, b->dFloat.ptr, n8);
            HIP_TRY(hipGetLastError());
        }
        b->floatFresh = true;
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (fetch_results(b)) return -1;
    long long n = std::min<long long>(b->results[u].produced, capacity);
    if (n > 0) HIP_TRY(hipMemcpy(sampleBuf, b->dFloat.ptr + b->outStart[u], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

int speechPlayer_batch_digest(speechPlayer_batch_t batch, unsigned long long* perUtterance, unsigned long long* whole)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) { set_error("digest: no batch"); return -1; }
    HIP_TRY(hipSetDevice(b->device));
    std::vector<unsigned long long> host((size_t)b->nUtt);
    if (b->nUtt) {
        if (b->dDigest.reserve((size_t)b->nUtt)) return -1;
        const unsigned grid = (unsigned)std::min<long long>((b->nUtt + 3) / 4, 16384);
        hipLaunchKernelGGL(pcm_digest, dim3(grid), dim3(256), 0, b->stream, b->dPcm.ptr, b->dUtt.ptr, b->dResult.ptr, b->dDigest.ptr, b->nUtt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host.data(), b->dDigest.ptr, (size_t)b->nUtt * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    if (perUtterance && b->nUtt) memcpy(perUtterance, host.data(), (size_t)b->nUtt * sizeof(unsigned long long));
    if (whole) {
        unsigned long long acc = 0;
        for (long long u = 0; u < b->nUtt; ++u) acc += digest_mix((unsigned long long)u, 0u) ^ host[u] * 0x9E3779B97F4A7C15ull;
        *whole = acc;
    }
    return 0;
}

int speechPlayer_batch_getLastIndex(speechPlayer_batch_t batch, long long u)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt) return -1;
    if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) return -1;
    if (fetch_results(b)) return -1;
    return b->results[u].lastIndex;
}

const sample* speechPlayer_batch_devicePcm(speechPlayer_batch_t batch)
{
    Batch* b = static_cast<Batch*>(batch);
    return b ? reinterpret_cast<const sample*>(b->dPcm.ptr) : nullptr;
}

long long speechPlayer_batch_deviceOffset(speechPlayer_batch_t batch, long long u)
{
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u > b->nUtt) return -1;
    return b->outStart[u];
}

int speechPlayer_batch_device(speechPlayer_batch_t batch)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) { set_error("batch_device: no batch"); return -1; }
    return b->device;
}

// The chosen utterances' PCM into the caller's device memory on the caller's stream (pcm_export), ordered by events only: behind the
// batch's last synthesis launch (pcmReady on `stream`, which every launch joins its side streams into), and ahead of the batch's next
// launch or set call (wait_exports).  The rows' descriptors are staged through a page-locked slot; nothing waits on the host unless
// all kExportSlots slots still hold exports in flight.
long long speechPlayer_batch_exportPcm(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, void* deviceOut,
                                       int format, long long rowStride, void* stream)
{
    begin_call();
    if (refuse_timing_only("speechPlayer_batch_exportPcm")) return -1;
    return batch_entry("exportPcm", batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportPcm: format %d (0 int16, 1 float32)", format); return -1; }
        if (rowStride < 0) { set_error("exportPcm: rowStride %lld", rowStride); return -1; }
        const bool packed = rowStride == 0;
        std::vector<ExportRow> rows;
        ExportSelection s;
        if (export_selection(b, "exportPcm", utterances, nUtterances, false, s, [&](long long, long long u, long long) {
                rows.push_back(ExportRow{b->outStart[(size_t)u], (long long)b->lens[(size_t)u]});
                return rows.back().len;
            })) return -1;
        const long long n = s.n, maxLen = s.most, total = s.total;
        std::vector<long long> words;      // the rows' starts in the output and the chunks' first rows (packed)
        const RowTable table = packed ? packed_row_table(s.counts.data(), 0, n, kExportChunkLog2, words) : RowTable{0, 0};
        if (!packed && rowStride < maxLen) { set_error("exportPcm: rowStride %lld is below the longest chosen utterance (%lld samples)", rowStride, maxLen); return -1; }
        if (!packed && n > (1ll << 50) / rowStride) { set_error("exportPcm: %lld rows of %lld elements", n, rowStride); return -1; }
        const long long elements = packed ? total : n * rowStride;
        if (elements == 0) return 0;
        if (!b->launched) { set_error("exportPcm: the batch has not been synthesised since it was set"); return -1; }
        const size_t elSize = format ? sizeof(float) : sizeof(int16_t);
        HIP_TRY(hipSetDevice(b->device));
        if (!deviceOut) { set_error("exportPcm: no output buffer"); return -1; }
        if (!device_range(deviceOut, (size_t)elements * elSize, b->device, elSize, "exportPcm")) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        Batch::ExportSlot& slot = b->exportSlot[b->exportNext++ % Batch::kExportSlots];
        if (slot.used) { HIP_TRY(hipEventSynchronize(slot.done)); slot.used = false; }
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        if (slot.host.ensure(block.bytes()) || slot.dev.reserve(block.bytes())) return -1;
        block.copy_to(slot.host.ptr);
        HIP_TRY(hipMemcpyAsync(slot.dev.ptr, slot.host.ptr, block.bytes(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(b->pcmReady, b->stream));
        HIP_TRY(hipStreamWaitEvent(st, b->pcmReady, 0));
        const ExportRow* dRows = block.device<ExportRow>(rowsAt, slot.dev.ptr);
        const long long* dDst = packed ? block.device<long long>(wordsAt, slot.dev.ptr) + table.startOff : nullptr;
        const long long* dChunk = packed ? block.device<long long>(wordsAt, slot.dev.ptr) + table.chunkOff : nullptr;
        const long long n8 = (elements + 7) / 8;
        const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 8ll * b->cus);
        const int vec = reinterpret_cast<uintptr_t>(deviceOut) % 16 == 0;
        if (format) hipLaunchKernelGGL(pcm_export<true>, dim3(grid), dim3(256), 0, st, b->dPcm.ptr, deviceOut, dRows, dDst, dChunk, n, rowStride, elements, vec);
        else hipLaunchKernelGGL(pcm_export<false>, dim3(grid), dim3(256), 0, st, b->dPcm.ptr, deviceOut, dRows, dDst, dChunk, n, rowStride, elements, vec);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(slot.done, st));
        slot.used = true;
        return elements;
    });
}

int speechPlayer_batch_time(speechPlayer_batch_t batch, int launches, float* msPerLaunch)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || launches <= 0 || !msPerLaunch) return -1;
    HIP_TRY(hipSetDevice(b->device));
    struct Events {
        std::vector<hipEvent_t> v;
        ~Events() { for (auto e : v) if (e) (void)hipEventDestroy(e); }
    } events;
    events.v.assign((size_t)launches * 2, nullptr);
    std::vector<hipEvent_t>& ev = events.v;
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    int rc = 0;
    for (int i = 0; i < launches && !rc; ++i) {
        HIP_TRY(hipEventRecord(ev[2 * i], b->stream));
        rc = batch_launch(b);
        HIP_TRY(hipEventRecord(ev[2 * i + 1], b->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int i = 0; i < launches && !rc; ++i) HIP_TRY(hipEventElapsedTime(&msPerLaunch[i], ev[2 * i], ev[2 * i + 1]));
    return rc;
}

// ==========================================================================================
// C-ABI: one batch over several devices of a node
// ==========================================================================================
// Utterances are independent, so a node's batch is cut into contiguous shards with near-equal total SAMPLE counts
// (closed-form lengths; what balances the kernels is samples, not utterance counts), one shard per device, each shard a
// Batch of its own with its own stream.  One host thread per device uploads its shard; launches are asynchronous, so
// every device synthesises at the same time; nothing is exchanged between devices (no collective).
struct Node {
    int sampleRate = 0;
    std::vector<Batch*> parts;
    std::vector<long long> bounds;       // contiguous deal: shard d = utterances bounds[d] .. bounds[d + 1] - 1
    int deal = 0;                        // option "deal": 0 contiguous shards of near-equal sample count, 1 the sorted deal
    bool sorted = false;                 // the batch that is set was dealt sorted: shard d = members[d]
    std::vector<std::vector<long long>> members;   // sorted deal: the utterances of every shard, in the shard's own order
    std::vector<int> shardOf;            // sorted deal: [nUtterances]
    std::vector<long long> localOf;      // ... and the utterance's number within its shard
    long long nUtt = 0;
};

speechPlayer_node_t speechPlayer_node_create(int sampleRate, int nDevices, const int* devices)
{
    begin_call();
    if (nDevices <= 0) { set_error("node_create: need at least one device"); return nullptr; }
    Node* n = new Node;
    n->sampleRate = sampleRate;
    for (int d = 0; d < nDevices; ++d) {
        Batch* b = static_cast<Batch*>(speechPlayer_batch_create(sampleRate, devices ? devices[d] : d));
        if (!b) { speechPlayer_node_destroy(n); return nullptr; }
        n->parts.push_back(b);
    }
    n->bounds.assign((size_t)nDevices + 1, 0);
    return n;
}

void speechPlayer_node_destroy(speechPlayer_node_t node)
{
    Node* n = static_cast<Node*>(node);
    if (!n) return;
    for (Batch* b : n->parts) speechPlayer_batch_destroy(b);
    delete n;
}

int speechPlayer_node_devices(speechPlayer_node_t node) { return node ? (int)static_cast<Node*>(node)->parts.size() : -1; }

speechPlayer_batch_t speechPlayer_node_part(speechPlayer_node_t node, int shard)
{
    Node* n = static_cast<Node*>(node);
    return (n && shard >= 0 && shard < (int)n->parts.size()) ? n->parts[shard] : nullptr;
}

int speechPlayer_node_setOption(speechPlayer_node_t node, const char* name, int value)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n || !name) return -1;
    // "deal" (read by speechPlayer_node_setUtterances): 0 contiguous shards of near-equal total sample count (default), 1 the SORTED deal
    // of SURVEY 8(e): utterances sorted by length, blocks of 64 (one wavefront) dealt round-robin, so that every device sees the same
    // length distribution -- a batch whose long utterances cluster gives every device its share of them.  Results are addressed by the
    // batch's own utterance numbers either way.
    if (!strcmp(name, "deal")) { n->deal = value ? 1 : 0; return 0; }
    for (Batch* b : n->parts)
        if (speechPlayer_batch_setOption(b, name, value)) return -1;
    return 0;
}

// The deal of a node's batch: before[u] = samples before utterance u (closed-form lengths).  Contiguous shards of near-equal
// sample count, or -- option "deal" -- the sorted deal: longest first (ties in the batch's order), blocks of 64 dealt round-robin
// (nvspeechplayer_amd.sharding.shard_deal states the same rules).
static void node_deal(Node* n, long long nUtterances, const std::vector<unsigned long long>& before)
{
    const int nd = (int)n->parts.size();
    const unsigned long long total = before[nUtterances];
    n->nUtt = nUtterances;
    n->sorted = n->deal == 1 && nd > 1;
    n->members.clear(); n->shardOf.clear(); n->localOf.clear();
    n->bounds[0] = 0;
    for (int d = 1; d < nd; ++d) {
        // first utterance whose start is at or beyond d/nd of the samples (the rule of nvspeechplayer_amd.sharding.shard_bounds)
        const double target = (double)total * d / (double)nd;
        long long cut = std::lower_bound(before.begin(), before.end(), target, [](unsigned long long x, double t) { return (double)x < t; }) - before.begin();
        n->bounds[d] = std::max(n->bounds[d - 1], std::min(cut, nUtterances));
    }
    n->bounds[nd] = nUtterances;
    if (n->sorted) {
        // longest first (ties in the batch's order), blocks of 64 dealt round-robin (nvspeechplayer_amd.sharding.shard_deal states the same rule)
        std::vector<long long> order((size_t)nUtterances);
        std::iota(order.begin(), order.end(), 0ll);
        std::stable_sort(order.begin(), order.end(), [&](long long x, long long y) { return before[x + 1] - before[x] > before[y + 1] - before[y]; });
        n->members.assign((size_t)nd, {});
        n->shardOf.assign((size_t)nUtterances, 0); n->localOf.assign((size_t)nUtterances, 0);
        for (long long i = 0; i < nUtterances; ++i) {
            const int d = (int)((i / kLanes) % nd);
            n->shardOf[(size_t)order[i]] = d;
            n->localOf[(size_t)order[i]] = (long long)n->members[(size_t)d].size();
            n->members[(size_t)d].push_back(order[i]);
        }
    }
}

int speechPlayer_node_setUtterances(speechPlayer_node_t node, long long nUtterances, const long long* frameStart,
                                    const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration,
                                    const unsigned int* fadeDuration, const int* userIndex, const unsigned char* isNull,
                                    const unsigned int* noiseSeed)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n || nUtterances < 0 || !frameStart) { set_error("node_setUtterances: bad arguments"); return -1; }
    if (frameStart[0] != 0) { set_error("node_setUtterances: frameStart[0] must be 0"); return -1; }
    for (long long u = 0; u < nUtterances; ++u)
        if (frameStart[u + 1] < frameStart[u]) { set_error("node_setUtterances: frameStart not monotone at %lld", u); return -1; }
    if (frameStart[nUtterances] > 0 && (!minFrameDuration || !fadeDuration)) { set_error("node_setUtterances: bad frame arrays"); return -1; }
    // samples before each utterance (closed form: a request spans max(M, F + 1) + 1 samples, F clamped to >= 1)
    std::vector<unsigned long long> before((size_t)nUtterances + 1, 0);
    for (long long u = 0; u < nUtterances; ++u) {
        unsigned long long len = 0;
        for (long long k = frameStart[u]; k < frameStart[u + 1]; ++k) {
            const unsigned long long m = minFrameDuration[k], f = std::max(fadeDuration[k], 1u);
            len += std::max(m, f + 1) + 1;
        }
        before[u + 1] = before[u] + len;
    }
    node_deal(n, nUtterances, before);
    const int nd = (int)n->parts.size();
    // one host thread per device: rebase the shard's index array, give every utterance its GLOBAL default seed, upload
    std::vector<int> rc((size_t)nd, 0), codes((size_t)nd, 0);
    std::vector<std::string> errors((size_t)nd);
    // (run_parts: a thread that cannot be started leaves its shard to the caller's thread; nothing may throw across the C ABI)
    try {
    run_parts((unsigned)nd, [&](unsigned ud) {
        const int d = (int)ud;
        try {
            if (n->sorted) {
                // the shard's utterances are scattered over the batch: their frames are gathered (one copy on the host, 392 bytes per frame)
                const std::vector<long long>& mem = n->members[(size_t)d];
                std::vector<long long> fs(mem.size() + 1, 0);
                for (size_t j = 0; j < mem.size(); ++j) fs[j + 1] = fs[j] + (frameStart[mem[j] + 1] - frameStart[mem[j]]);
                const size_t nf = (size_t)fs[mem.size()];
                std::vector<speechPlayer_frame_t> fr(frames ? nf : 0);
                std::vector<unsigned int> mins(nf), fades(nf), seeds(mem.size());
                std::vector<int> idx(userIndex ? nf : 0);
                std::vector<unsigned char> nul(isNull ? nf : 0);
                for (size_t j = 0; j < mem.size(); ++j) {
                    const long long a = frameStart[mem[j]], cnt = frameStart[mem[j] + 1] - a, at = fs[j];
                    if (cnt > 0) {
                        if (frames) memcpy(&fr[(size_t)at], frames + a, (size_t)cnt * sizeof(speechPlayer_frame_t));
                        memcpy(&mins[(size_t)at], minFrameDuration + a, (size_t)cnt * sizeof(unsigned int));
                        memcpy(&fades[(size_t)at], fadeDuration + a, (size_t)cnt * sizeof(unsigned int));
                        if (userIndex) memcpy(&idx[(size_t)at], userIndex + a, (size_t)cnt * sizeof(int));
                        if (isNull) memcpy(&nul[(size_t)at], isNull + a, (size_t)cnt);
                    }
                    seeds[j] = noiseSeed ? noiseSeed[mem[j]] : (unsigned int)mem[j];
                }
                rc[d] = speechPlayer_batch_setUtterances(n->parts[d], (long long)mem.size(), fs.data(), frames ? fr.data() : nullptr, mins.data(), fades.data(),
                                                         userIndex ? idx.data() : nullptr, isNull ? nul.data() : nullptr, seeds.data());
                if (rc[d]) { errors[d] = g_lastError; codes[d] = g_lastErrorCode; }
                return;
            }
            const long long u0 = n->bounds[d], u1 = n->bounds[d + 1], f0 = frameStart[u0];
            std::vector<long long> fs((size_t)(u1 - u0) + 1);
            for (long long u = u0; u <= u1; ++u) fs[u - u0] = frameStart[u] - f0;
            std::vector<unsigned int> seeds((size_t)(u1 - u0));
            for (long long u = u0; u < u1; ++u) seeds[u - u0] = noiseSeed ? noiseSeed[u] : (unsigned int)u;
            rc[d] = speechPlayer_batch_setUtterances(n->parts[d], u1 - u0, fs.data(), frames ? frames + f0 : nullptr,
                                                     minFrameDuration ? minFrameDuration + f0 : nullptr, fadeDuration ? fadeDuration + f0 : nullptr,
                                                     userIndex ? userIndex + f0 : nullptr, isNull ? isNull + f0 : nullptr, seeds.data());
            if (rc[d]) { errors[d] = g_lastError; codes[d] = g_lastErrorCode; }
        } catch (const std::exception& e) {
            rc[d] = -1; errors[d] = e.what(); codes[d] = SPEECHPLAYER_ERR_ARGUMENT;
        }
    });
    } catch (const std::exception& e) {
        set_error("node_setUtterances: %s", e.what());
        return -1;
    }
    for (int d = 0; d < nd; ++d)
        if (rc[d]) { set_error_code(codes[d]); set_error("node_setUtterances: shard %d: %s", d, errors[d].c_str()); return -1; }
    return 0;
}

// The node's batch in compact form (speechPlayer_batch_setRecords): the lists, their records and the shape table go to EVERY shard (they
// are small), each shard gets the utterances the deal gives it -- their list numbers and noise seeds.
int speechPlayer_node_setRecords(speechPlayer_node_t node, long long nShapes, const speechPlayer_frame_t* shapes, long long nLists,
                                 const long long* listStart, const speechPlayer_frameRecord_t* records, long long nUtterances,
                                 const unsigned int* listOf, const unsigned int* noiseSeed)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n || nUtterances < 0 || nLists < 0 || !listStart) { set_error("node_setRecords: bad arguments"); return -1; }
    if (!listOf && nUtterances != nLists) { set_error("node_setRecords: %lld utterances for %lld lists and no listOf", nUtterances, nLists); return -1; }
    if (listStart[0] != 0) { set_error("node_setRecords: listStart[0] must be 0"); return -1; }
    for (long long l = 0; l < nLists; ++l)
        if (listStart[l + 1] < listStart[l]) { set_error("node_setRecords: listStart not monotone at %lld", l); return -1; }
    if (listStart[nLists] > 0 && !records) { set_error("node_setRecords: no records"); return -1; }
    for (long long u = 0; listOf && u < nUtterances; ++u)
        if ((long long)listOf[u] >= nLists) { set_error("node_setRecords: listOf[%lld] is not a list", u); return -1; }
    try {
        std::vector<unsigned long long> lenL((size_t)nLists, 0), before((size_t)nUtterances + 1, 0);
        for (long long l = 0; l < nLists; ++l)
            for (long long k = listStart[l]; k < listStart[l + 1]; ++k) {
                const unsigned long long m = records[k].minFrameDuration, f = std::max(records[k].fadeDuration, 1u);
                lenL[(size_t)l] += std::max(m, f + 1) + 1;
            }
        for (long long u = 0; u < nUtterances; ++u) before[(size_t)u + 1] = before[(size_t)u] + lenL[listOf ? listOf[u] : (size_t)u];
        node_deal(n, nUtterances, before);
        const int nd = (int)n->parts.size();
        std::vector<int> rc((size_t)nd, 0), codes((size_t)nd, 0);
        std::vector<std::string> errors((size_t)nd);
        run_parts((unsigned)nd, [&](unsigned ud) {
            const int d = (int)ud;
            try {
                const long long cnt = n->sorted ? (long long)n->members[(size_t)d].size() : n->bounds[d + 1] - n->bounds[d];
                std::vector<unsigned int> lo((size_t)cnt), seeds((size_t)cnt);
                for (long long j = 0; j < cnt; ++j) {
                    const long long u = n->sorted ? n->members[(size_t)d][(size_t)j] : n->bounds[d] + j;
                    lo[(size_t)j] = listOf ? listOf[u] : (unsigned int)u;
                    seeds[(size_t)j] = noiseSeed ? noiseSeed[u] : (unsigned int)u;
                }
                rc[d] = speechPlayer_batch_setRecords(n->parts[d], nShapes, shapes, nLists, listStart, records, cnt, lo.data(), seeds.data());
                if (rc[d]) { errors[d] = g_lastError; codes[d] = g_lastErrorCode; }
            } catch (const std::exception& e) {
                rc[d] = -1; errors[d] = e.what(); codes[d] = SPEECHPLAYER_ERR_ARGUMENT;
            }
        });
        for (int d = 0; d < nd; ++d)
            if (rc[d]) { set_error_code(codes[d]); set_error("node_setRecords: shard %d: %s", d, errors[d].c_str()); return -1; }
    } catch (const std::exception& e) {
        set_error("node_setRecords: %s", e.what());
        return -1;
    }
    return 0;
}

int speechPlayer_node_synthesize(speechPlayer_node_t node)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n) return -1;
    for (Batch* b : n->parts) {       // asynchronous launches: the devices run side by side
        HIP_TRY(hipSetDevice(b->device));
        if (batch_launch(b)) return -1;
    }
    return 0;
}

int speechPlayer_node_wait(speechPlayer_node_t node)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n) return -1;
    for (Batch* b : n->parts) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return 0;
}

int speechPlayer_node_shardInfo(speechPlayer_node_t node, int shard, long long* firstUtterance, long long* nUtterances, long long* samples, int* device)
{
    Node* n = static_cast<Node*>(node);
    if (!n || shard < 0 || shard >= (int)n->parts.size()) return -1;
    if (firstUtterance) *firstUtterance = n->sorted ? -1 : n->bounds[shard];      // (the sorted deal's shards are not ranges: speechPlayer_node_shardUtterances)
    if (nUtterances) *nUtterances = n->sorted ? (long long)n->members[(size_t)shard].size() : n->bounds[shard + 1] - n->bounds[shard];
    if (samples) *samples = n->parts[shard]->totalSamples;
    if (device) *device = n->parts[shard]->device;
    return 0;
}

long long speechPlayer_node_totalSamples(speechPlayer_node_t node)
{
    Node* n = static_cast<Node*>(node);
    if (!n) return -1;
    long long t = 0;
    for (Batch* b : n->parts) t += b->totalSamples;
    return t;
}

// the shard that holds utterance u and its number there
static int node_locate(Node* n, long long u, long long* local)
{
    if (!n || u < 0 || u >= n->nUtt) return -1;
    if (n->sorted) { *local = n->localOf[(size_t)u]; return n->shardOf[(size_t)u]; }
    const int d = (int)(std::upper_bound(n->bounds.begin(), n->bounds.end(), u) - n->bounds.begin()) - 1;
    *local = u - n->bounds[d];
    return d;
}

long long speechPlayer_node_shardUtterances(speechPlayer_node_t node, int shard, long long* utterances, long long capacity)
{
    Node* n = static_cast<Node*>(node);
    if (!n || shard < 0 || shard >= (int)n->parts.size()) return -1;
    const long long cnt = n->sorted ? (long long)n->members[(size_t)shard].size() : n->bounds[shard + 1] - n->bounds[shard];
    if (utterances && cnt <= capacity)
        for (long long j = 0; j < cnt; ++j) utterances[j] = n->sorted ? n->members[(size_t)shard][(size_t)j] : n->bounds[shard] + j;
    return cnt;
}

long long speechPlayer_node_read(speechPlayer_node_t node, long long u, sample* sampleBuf, long long capacity)
{
    Node* n = static_cast<Node*>(node);
    long long local = 0;
    const int d = node_locate(n, u, &local);
    if (d < 0) { begin_call(); set_error("node_read: utterance %lld out of range", u); return -1; }
    return speechPlayer_batch_read(n->parts[d], local, sampleBuf, capacity);
}

int speechPlayer_node_getLastIndex(speechPlayer_node_t node, long long u)
{
    Node* n = static_cast<Node*>(node);
    long long local = 0;
    const int d = node_locate(n, u, &local);
    return d < 0 ? -1 : speechPlayer_batch_getLastIndex(n->parts[d], local);
}

// `launches` passes over the node's batch, every device launched before any is waited for; wall-clock milliseconds per pass
int speechPlayer_node_time(speechPlayer_node_t node, int launches, float* msPerLaunch)
{
    begin_call();
    Node* n = static_cast<Node*>(node);
    if (!n || launches <= 0 || !msPerLaunch) return -1;
    if (speechPlayer_node_wait(n)) return -1;
    for (int i = 0; i < launches; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        if (speechPlayer_node_synthesize(n) || speechPlayer_node_wait(n)) return -1;
        msPerLaunch[i] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

// diagnostic builds (-DKLATT_STAMPS): per workgroup and stage {work cycles, barrier-wait cycles} of the last launch
int speechPlayer_batch_debugStamps(speechPlayer_batch_t batch, unsigned long long* out, int capacity)
{
    Batch* b = static_cast<Batch*>(batch);
    if (!b || !out) return -1;
    int n = (int)std::min<size_t>(b->dDebug.cap, (size_t)capacity);
    if (n > 0) HIP_TRY(hipMemcpy(out, b->dDebug.ptr, (size_t)n * 8, hipMemcpyDeviceToHost));
    return n;
}

int speechPlayer_batch_kernelInfo(speechPlayer_batch_t batch, int* info, int nInfo)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || !info || nInfo < 6) return -1;
    HIP_TRY(hipSetDevice(b->device));
    hipFuncAttributes fa;
    // report the kernel of the largest of the three groups (batch_launch)
    const long long nNoisy = b->nSlots - b->nQuiet, nLp = lanepipe_count(b);
    const long long nNn = b->layout == 0 ? 0 : b->nNoNasal - nLp, nQ = b->nQuiet - nLp - nNn;
    const bool lanepipe = nLp > 0 && nLp >= nQ && nLp >= nNoisy && nLp >= nNn;
    const bool nasalFree = !lanepipe && nNn > 0 && nNn >= nQ && nNn >= nNoisy;
    const bool noisy = !lanepipe && !nasalFree && nNoisy >= nQ;
    const GroupPlan pl = plan_group(b->layout, noisy, b->nSlots, nNoisy, b->cus);
    const bool fast = b->mode == MODE_FAST;
    const long long nTr = tracked_count(b);
    const long long nDir = direct_count(b);
    const bool directG = noisy && nDir > 0 && nDir >= nTr && nDir >= nNoisy - nTr - nDir;
    const bool tracked = noisy && !directG && nTr > 0 && nTr >= nNoisy - nTr - nDir;
    const void* fn;
    int ldsBytes = LdsLayout<false>::kBytes, chunk = 0, wavesPerGroup = 1;
    long long groups = (nNn + kLanes - 1) / kLanes + (nQ + kLanes - 1) / kLanes + (nNoisy + kLanes - 1) / kLanes;
    if (nasalFree) {
        if (pl.chunk == 32) { fn = fast ? (const void*)klatt_systolic<MODE_FAST, false, 32, 1, false> : (const void*)klatt_systolic<MODE_EXACT, false, 32, 1, false>; ldsBytes = SysLds<false, 32>::kBytes; }
        else { fn = fast ? (const void*)klatt_systolic<MODE_FAST, false, 16, 2, false> : (const void*)klatt_systolic<MODE_EXACT, false, 16, 2, false>; ldsBytes = SysLds<false, 16>::kBytes; }
        chunk = pl.chunk;
        wavesPerGroup = kStages;
    } else if (lanepipe) {
        const long long g = (nLp + kLpUPG - 1) / kLpUPG;
        if (g <= b->cus) { fn = fast ? (const void*)klatt_lanepipe<MODE_FAST, KLATT_LP_CH, 1> : (const void*)klatt_lanepipe<MODE_EXACT, KLATT_LP_CH, 1>; ldsBytes = LpLds<KLATT_LP_CH>::kBytes; chunk = KLATT_LP_CH; }
        else { fn = fast ? (const void*)klatt_lanepipe<MODE_FAST, 16, 2> : (const void*)klatt_lanepipe<MODE_EXACT, 16, 2>; ldsBytes = LpLds<16>::kBytes; chunk = 16; }
        wavesPerGroup = kStages;
        groups = g;
    } else if (directG) {
        if (direct_lean(b, (nDir + kLanes - 1) / kLanes)) {
            fn = fast ? (const void*)klatt_direct<MODE_FAST, kDirectLeanChunk, 4> : (const void*)klatt_direct<MODE_EXACT, kDirectLeanChunk, 4>;
            ldsBytes = DirectLds<kDirectLeanChunk>::kBytes; chunk = kDirectLeanChunk;
        } else {
            fn = fast ? (const void*)klatt_direct<MODE_FAST, kDirectChunk, 2> : (const void*)klatt_direct<MODE_EXACT, kDirectChunk, 2>;
            ldsBytes = DirectLds<kDirectChunk>::kBytes; chunk = kDirectChunk;
        }
        wavesPerGroup = kDirectStages;
    } else if (tracked) {
        if (pl.chunk == 8) { fn = fast ? (const void*)klatt_systolic<MODE_FAST, true, KLATT_FLAT_CH, KLATT_FLAT_WPS, true, false, true> : (const void*)klatt_systolic<MODE_EXACT, true, KLATT_FLAT_CH, KLATT_FLAT_WPS, true, false, true>; ldsBytes = SysLds<true, KLATT_FLAT_CH, true>::kBytes; chunk = KLATT_FLAT_CH; }
        else { fn = fast ? (const void*)klatt_systolic<MODE_FAST, true, 16, 1, true, false, true> : (const void*)klatt_systolic<MODE_EXACT, true, 16, 1, true, false, true>; ldsBytes = SysLds<true, 16, true>::kBytes; chunk = 16; }
        wavesPerGroup = kStages;
    } else if (pl.systolic) {
        if (noisy && pl.chunk == 8) { fn = fast ? (const void*)klatt_systolic<MODE_FAST, true, 8, 2> : (const void*)klatt_systolic<MODE_EXACT, true, 8, 2>; ldsBytes = SysLds<true, 8>::kBytes; }
        else if (noisy) { fn = fast ? (const void*)klatt_systolic<MODE_FAST, true, 16> : (const void*)klatt_systolic<MODE_EXACT, true, 16>; ldsBytes = SysLds<true, 16>::kBytes; }
        else if (pl.chunk == 32) { fn = fast ? (const void*)klatt_systolic<MODE_FAST, false, 32> : (const void*)klatt_systolic<MODE_EXACT, false, 32>; ldsBytes = SysLds<false, 32>::kBytes; }
        else { fn = fast ? (const void*)klatt_systolic<MODE_FAST, false, 16> : (const void*)klatt_systolic<MODE_EXACT, false, 16>; ldsBytes = SysLds<false, 16>::kBytes; }
        chunk = pl.chunk;
        wavesPerGroup = kStages;
    } else {
        fn = fast ? (noisy ? (const void*)klatt_synthesize<MODE_FAST, false, true> : (const void*)klatt_synthesize<MODE_FAST, false, false>)
                  : (noisy ? (const void*)klatt_synthesize<MODE_EXACT, false, true> : (const void*)klatt_synthesize<MODE_EXACT, false, false>);
    }
    HIP_TRY(hipFuncGetAttributes(&fa, fn));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, b->device));
    info[0] = fa.numRegs;
    info[1] = ldsBytes;
    info[2] = (int)(groups * wavesPerGroup);
    info[3] = prop.multiProcessorCount;
    info[4] = (int)(prop.sharedMemPerMultiprocessor / ldsBytes);
    info[5] = (int)fa.localSizeBytes;   // scratch
    if (nInfo >= 8) { info[6] = chunk; info[7] = noisy ? 1 : 0; }
    // (utterances, not slots: the lane-pipelined kernel takes all of the nasal-free group or none of it)
    if (nInfo >= 10) { info[8] = lanepipe ? 1 : 0; info[9] = (int)std::min<long long>(nLp > 0 ? b->nNoNasalUtt : 0, 0x7FFFFFFF); }
    if (nInfo >= 12) { info[10] = nasalFree ? 1 : 0; info[11] = (int)std::min<long long>(nNn > 0 ? b->nNoNasalUtt : 0, 0x7FFFFFFF); }
    if (nInfo >= 16) {
        info[12] = (int)std::min<long long>(nTr > 0 ? b->nTrackedUtt : 0, 0x7FFFFFFF); info[13] = (int)std::min<long long>(b->nJobs, 0x7FFFFFFF);
        info[14] = (int)std::min<long long>(b->trackEntries * (long long)sizeof(double2) >> 20, 0x7FFFFFFF); info[15] = tracked ? 1 : 0;
    }
    if (nInfo >= 20) {
        info[16] = (int)std::min<long long>(b->nDirectUtt, 0x7FFFFFFF); info[17] = directG ? 1 : 0;
        info[18] = (int)std::min<long long>(b->nDirectFrames * (long long)(kDirectEntries * sizeof(double2) + kDirectStages * sizeof(DirectHdr)) >> 20, 0x7FFFFFFF);
        info[19] = 0;
    }
    if (nInfo >= 23) {
        // the LAST launch's wavefronts (one per workgroup and stage) that ran without parallel 1 / turbulence / the aspiration generator, counted
        // by the stages themselves; before the first launch of a batch: what the plan says they will be under the option as it stands.
        // Behind them (nInfo >= 23 + kDead2Counts), the same way: the wavefronts whose source stage ran without turbulence and the nasal pair,
        // whose final stage ran without parallel 5 / without parallel 5 and 6, whose parallel stage ran without parallel 1..4 (dead2_wave_counts).
        constexpr int kAll = 3 + kDead2Counts;
        uint32_t dead[kAll] = {};
        if (b->launched && nTr > 0 && b->dDeadWaves.ptr) {
            HIP_TRY(hipStreamSynchronize(b->stream));      // (every launch joins its side streams into this one)
            HIP_TRY(hipMemcpy(dead, b->dDeadWaves.ptr, sizeof dead, hipMemcpyDeviceToHost));      // one copy of the counters' block
        } else if (nTr > 0 && b->deadTerms) {
            for (int k = 0; k < 3; ++k) dead[k] = (uint32_t)std::min<long long>(b->planDeadWaves[k], 0x7FFFFFFFll);
            for (int k = 0; k < kDead2Counts; ++k) dead[3 + k] = (uint32_t)std::min<long long>(b->planDead2Waves[k], 0x7FFFFFFFll);
        }
        const int n = nInfo >= 20 + kAll ? kAll : 3;
        for (int k = 0; k < n; ++k) info[20 + k] = (int)std::min<uint32_t>(dead[k], 0x7FFFFFFFu);
    }
    return 0;
}


// Host-only view of the track planning (tests, tools): the plan speechPlayer_batch_setUtterances would make for these
// utterances (eligible[u] != 0: utterance u may be tracked; NULL: all).  Per frame: first entry and resonator mask of its
// fade's track (0 / 0 in utterances that are not tracked); per utterance: tracked or not.  Returns the number of distinct
// tracks, *nEntries the 16-byte entries they hold; -1 on bad arguments.  Touches no device.
static long long plan_tracks_view(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
                                  const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible,
                                  long long budgetMB, const void* facts24, unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked,
                                  unsigned long long* nEntries, long long* collisionAt, unsigned int* kinds = nullptr)
{
    begin_call();
    if (nUtterances < 0 || !frameStart || frameStart[0] != 0) { set_error("planTracks: bad arguments"); return -1; }
    for (long long u = 0; u < nUtterances; ++u)
        if (frameStart[u + 1] < frameStart[u]) { set_error("planTracks: frameStart not monotone at %lld", u); return -1; }
    const long long nF = frameStart[nUtterances];
    if (nF > 0 && (!frames || !fadeDuration)) { set_error("planTracks: bad frame arrays"); return -1; }
    std::vector<FrameMeta> meta((size_t)nF);
    for (long long k = 0; k < nF; ++k) {
        meta[k].minSamples = 0; meta[k].userIndex = -1;
        meta[k].fadeSamples = std::max(fadeDuration[k], 1u);
        meta[k].flags = (isNull && isNull[k]) ? FRAME_NULL : 0u;
    }
    std::vector<unsigned char> all;
    if (!eligible) { all.assign((size_t)nUtterances, 1); eligible = all.data(); }
    TrackPlan plan;
    std::vector<FrameFacts> own;
    const FrameFacts* facts = static_cast<const FrameFacts*>(facts24);
    if (!facts) {
        own.resize((size_t)nF);
        parallel_ranges(nF, 1 << 14, [&](long long a, long long e) { for (long long k = a; k < e; ++k) own[k] = frame_facts(reinterpret_cast<const double*>(frames + k), 1e300, 1e300); });
        facts = own.data();
    }
    plan_tracks(nUtterances, frameStart, FrameSource{frames, nullptr, nullptr}, facts, meta.data(), eligible, track_budget_entries(budgetMB), plan_hash_mask(), plan);
    // what klatt_verify_shared does on the device, here on the host: every frame recognised by its hash against the frame that stood for it
    if (collisionAt) *collisionAt = -1;
    for (long long k = 0; k < nF && !plan.rep.empty(); ++k) {
        const uint32_t r = plan.rep[(size_t)k];
        if (r == 0xFFFFFFFFu || (long long)r == k) continue;
        if (!shape_values_equal(reinterpret_cast<const double*>(frames + k), reinterpret_cast<const double*>(frames + r))) {
            if (collisionAt) *collisionAt = k;
            set_error("planTracks: frames %lld and %u carry one 128-bit shape hash and different values", k, r);
            return -2;
        }
    }
    for (long long k = 0; k < nF; ++k) {
        if (trackOff) trackOff[k] = plan.ref[k].off;
        if (trackMask) trackMask[k] = plan.ref[k].mask;
    }
    // references of utterances that ended up untracked mean nothing: clear them
    for (long long u = 0; u < nUtterances; ++u) {
        if (tracked) tracked[u] = plan.tracked[u];
        if (kinds) kinds[u] = plan.tracked[u] ? plan.kinds[u] : 0u;
        if (!plan.tracked[u])
            for (long long k = frameStart[u]; k < frameStart[u + 1]; ++k) { if (trackOff) trackOff[k] = 0; if (trackMask) trackMask[k] = 0; }
    }
    if (nEntries) *nEntries = plan.entries;
    return (long long)plan.jobs.size();
}

long long speechPlayer_planTracks(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
                                  const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible,
                                  long long budgetMB, unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked,
                                  unsigned long long* nEntries)
{
    try {
        return plan_tracks_view(nUtterances, frameStart, frames, fadeDuration, isNull, eligible, budgetMB, nullptr, trackOff, trackMask, tracked, nEntries, nullptr);
    } catch (const std::exception& e) { set_error("planTracks: %s", e.what()); return -1; }
}

long long speechPlayer_planTracksFacts(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
                                       const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible,
                                       long long budgetMB, const void* facts24, unsigned long long* trackOff, unsigned int* trackMask,
                                       unsigned char* tracked, unsigned long long* nEntries, long long* collisionAt)
{
    try {
        return plan_tracks_view(nUtterances, frameStart, frames, fadeDuration, isNull, eligible, budgetMB, facts24, trackOff, trackMask, tracked, nEntries, collisionAt);
    } catch (const std::exception& e) { set_error("planTracksFacts: %s", e.what()); return -1; }
}

// The same plan, and per utterance the kinds word the flat stages get with it (TrackPlan::kinds, UttDesc.flags >> kUttKindShift):
// every entry kind whose value changes after the first sample of the utterance's first fade; 0 for an utterance that is not tracked.
long long speechPlayer_planTrackKinds(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
                                      const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible,
                                      long long budgetMB, unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked,
                                      unsigned long long* nEntries, unsigned int* kinds)
{
    try {
        return plan_tracks_view(nUtterances, frameStart, frames, fadeDuration, isNull, eligible, budgetMB, nullptr, trackOff, trackMask, tracked, nEntries, nullptr, kinds);
    } catch (const std::exception& e) { set_error("planTrackKinds: %s", e.what()); return -1; }
}

// the engine's worker threads for the other translation unit (frame_producer.cpp): fn(ctx, a, e) over [0, n) in ranges
void speechPlayer_internal_parallel(long long n, long long grain, void (*fn)(void* ctx, long long a, long long e), void* ctx)
{
    if (n <= 0 || !fn) return;
    parallel_ranges(n, grain, [&](long long a, long long e) { fn(ctx, a, e); });
}

// (This view reports the four facts a set call ROUTES by, FACT_NOISE .. FACT_UNBOUNDED, and the hash.  The "present" facts of the flat stages'
// dead terms travel in the same word inside the engine (klatt_consts.h); what they led to is reported per launch by speechPlayer_batch_kernelInfo.)
long long speechPlayer_frameFacts(const speechPlayer_frame_t* frames, long long nFrames, int sampleRate, int onDevice, void* facts24)
{
    begin_call();
    if (nFrames < 0 || (nFrames > 0 && (!frames || !facts24)) || sampleRate <= 0) { set_error("frameFacts: bad arguments"); return -1; }
    const double maxBw = 690.0 * sampleRate / M_PI, maxF = 9900.0 * sampleRate / (2.0 * M_PI);
    FrameFacts* const out = static_cast<FrameFacts*>(facts24);
    constexpr uint32_t kRouting = FACT_NOISE | FACT_NONFINITE | FACT_NASAL | FACT_UNBOUNDED;
    if (!onDevice) {
        parallel_ranges(nFrames, 1 << 13, [&](long long a, long long e) {
            for (long long k = a; k < e; ++k) { out[k] = frame_facts(reinterpret_cast<const double*>(frames + k), maxF, maxBw); out[k].flags &= kRouting; out[k].present2 = 0u; }
        });
        return nFrames;
    }
    if (nFrames == 0) return 0;
    DeviceBuffer<double> dF;
    DeviceBuffer<FrameFacts> dO;
    struct Release { DeviceBuffer<double>& a; DeviceBuffer<FrameFacts>& b; ~Release() { a.release(); b.release(); } } release{dF, dO};
    if (dF.reserve((size_t)nFrames * kNumParams) || dO.reserve((size_t)nFrames)) return -1;
    HIP_TRY(hipMemcpy(dF.ptr, frames, (size_t)nFrames * kNumParams * sizeof(double), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<long long>((nFrames + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(klatt_frame_facts, dim3(grid), dim3(256), 0, nullptr, dF.ptr, dO.ptr, nFrames, maxF, maxBw);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dO.ptr, (size_t)nFrames * sizeof(FrameFacts), hipMemcpyDeviceToHost));
    for (long long k = 0; k < nFrames; ++k) { out[k].flags &= kRouting; out[k].present2 = 0u; }
    return nFrames;
}

// Host-only view of what speechPlayer_batch_setUtterances hands klatt_seeds for the utterances it sends to the direct stages
// (tests; touches no device): per frame the frames its fade starts from and ends on (0xFFFFFFFF: none -- all zero) and the flags
// (bit 0: the start's preFormantGain is gated off, bit 1: the end's).  Returns the number of frames; -1 on bad arguments.
long long speechPlayer_planDirect(long long nUtterances, const long long* frameStart, const unsigned char* isNull,
                                  unsigned int* from, unsigned int* to, unsigned int* flags)
{
    begin_call();
    if (nUtterances < 0 || !frameStart || frameStart[0] != 0) { set_error("planDirect: bad arguments"); return -1; }
    for (long long u = 0; u < nUtterances; ++u)
        if (frameStart[u + 1] < frameStart[u]) { set_error("planDirect: frameStart not monotone at %lld", u); return -1; }
    const long long nF = frameStart[nUtterances];
    if (nF >= 0xFFFFFFFFll) { set_error("planDirect: too many frames"); return -1; }
    std::vector<FrameMeta> meta((size_t)nF);
    for (long long k = 0; k < nF; ++k) { meta[k].minSamples = 0; meta[k].fadeSamples = 1; meta[k].userIndex = -1; meta[k].flags = (isNull && isNull[k]) ? FRAME_NULL : 0u; }
    std::vector<DirectJob> jobs;
    jobs.reserve((size_t)nF);
    for (long long u = 0; u < nUtterances; ++u) walk_fade_ends(frameStart[u], frameStart[u + 1], meta.data(), jobs);
    for (long long k = 0; k < nF; ++k) {
        if (from) from[k] = jobs[(size_t)k].from;
        if (to) to[k] = jobs[(size_t)k].to;
        if (flags) flags[k] = jobs[(size_t)k].flags;
    }
    return nF;
}

// Host-only view of a batch's timeline (tests, tools, callers that plan before they set; touches no device): the sample every request
// is dequeued on and every utterance's length, from the durations alone (reference src/frame.cpp:41-80 with src/speechPlayer.cpp:36).
long long speechPlayer_planTimeline(long long nUtterances, const long long* frameStart, const unsigned int* minFrameDuration,
                                    const unsigned int* fadeDuration, long long* firstSample, long long* length)
{
    begin_call();
    if (nUtterances < 0 || !frameStart || frameStart[0] != 0) { set_error("planTimeline: bad arguments"); return -1; }
    for (long long u = 0; u < nUtterances; ++u)
        if (frameStart[u + 1] < frameStart[u]) { set_error("planTimeline: frameStart not monotone at %lld", u); return -1; }
    const long long nF = frameStart[nUtterances];
    if (nF > 0 && (!minFrameDuration || !fadeDuration)) { set_error("planTimeline: no durations"); return -1; }
    for (long long u = 0; u < nUtterances; ++u) {
        long long S = 0;
        for (long long k = frameStart[u]; k < frameStart[u + 1]; ++k) {
            if (firstSample) firstSample[k] = S;
            FrameMeta m;
            m.minSamples = minFrameDuration[k]; m.fadeSamples = std::max(fadeDuration[k], 1u);
            S += timeline_span(m);
        }
        if (length) length[u] = S;
    }
    return nF;
}

long long speechPlayer_batch_timeline(speechPlayer_batch_t batch, long long u, long long* firstSample, int* userIndex, long long capacity)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b || u < 0 || u >= b->nUtt) { set_error("batch_timeline: no such utterance"); return -1; }
    HIP_TRY(hipSetDevice(b->device));
    const long long n = b->uttFrames[(size_t)u], k0 = b->uttFrameStart[(size_t)u];
    if (n > capacity || (!firstSample && !userIndex)) return n;
    std::vector<FrameMeta> m((size_t)n);
    if (n) HIP_TRY(hipMemcpy(m.data(), b->dMeta.ptr + k0, (size_t)n * sizeof(FrameMeta), hipMemcpyDeviceToHost));
    long long S = 0;
    for (long long k = 0; k < n; ++k) {
        if (firstSample) firstSample[k] = S;
        if (userIndex) userIndex[k] = m[(size_t)k].userIndex;
        S += timeline_span(m[(size_t)k]);
    }
    if (firstSample) firstSample[n] = S;
    return n;
}

// ---- the exports of a batch as set ("the export path", above) ----------------------------------------------------------------------
// The batch's device, and the caller's output on it (zero elements have been answered before).
static int export_output(Batch* b, const char* what, void* deviceOut, long long elements, size_t elSize)
{
    HIP_TRY(hipSetDevice(b->device));
    if (!deviceOut) { set_error("%s: no output buffer", what); return -1; }
    return device_range(deviceOut, (size_t)elements * elSize, b->device, elSize, what) ? 0 : -1;
}

// An export of the batch's PCM needs a synthesis launch since the set call
static int export_synthesised(const Batch* b, const char* what)
{
    if (!b->launched) set_error("%s: the batch has not been synthesised since it was set", what);
    return b->launched ? 0 : -1;
}

// The arguments of the exports by step: hop and phase, and no utterance is longer than 2^32 samples: a larger hop or phase means the same.
static int step_request(const char* what, long long& hop, long long& phase, long long rowStride)
{
    if (hop <= 0 || phase < 0) { set_error("%s: hop %lld, phase %lld", what, hop, phase); return -1; }
    if (rowStride < 0) { set_error("%s: rowStride %lld", what, rowStride); return -1; }
    hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
    return 0;
}

static int column_range(const char* what, const int* columns, int nColumns, int known)
{
    for (int q = 0; q < nColumns; ++q)
        if (columns[q] < 0 || columns[q] >= known) { set_error("%s: columns[%d] = %d (0 .. %d)", what, q, columns[q], known - 1); return -1; }
    return 0;
}

// One row per chosen utterance for klatt_timeline_dense / klatt_source_dense, its steps counted.
static int step_rows(Batch* b, const char* what, const long long* utterances, long long nUtterances, long long hop, long long phase,
                     ExportSelection& s, std::vector<TimelineRow>& rows)
{
    return export_selection(b, what, utterances, nUtterances, true, s, [&](long long, long long u, long long) {
        rows.push_back(TimelineRow{b->uttFrameStart[(size_t)u], b->uttFrames[(size_t)u], 0, align_steps_below(b->lens[(size_t)u], hop, phase)});
        return rows.back().steps;
    });
}

// A dense kernel's launch over `elements` elements of elSize bytes from element `at` of the output: a lane per 16 bytes; the row table
// `t` of the packed form (null: padded) within the staged words.
struct DenseLaunch {
    char* out;
    unsigned grid;
    int vec;
    const long long *start, *chunk;
};
static DenseLaunch dense_launch(const Batch* b, void* deviceOut, long long at, long long elements, size_t elSize, const long long* dWords, const RowTable* t)
{
    DenseLaunch d;
    d.out = static_cast<char*>(deviceOut) + (size_t)at * elSize;
    const long long nLane = (elements * (long long)elSize + 15) / 16;
    d.grid = (unsigned)std::min<long long>((nLane + 255) / 256, 8ll * b->cus);
    d.vec = reinterpret_cast<uintptr_t>(d.out) % 16 == 0;
    d.start = t ? dWords + t->startOff : nullptr;
    d.chunk = t ? dWords + t->chunkOff : nullptr;
    return d;
}

// The tracks of chosen utterances (klatt_timeline.h).  An export that asks for column 0 walks the distinct lists its rows speak
// (klatt_timeline_pitch) into the voicePitch table, in pieces of rows whose lists fit option "pitch_table_mb"; one piece otherwise.
// The staging block: columns | rows | per piece: step starts and chunk rows (packed) | lists.
long long speechPlayer_batch_exportTracks(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const int* columns,
                                          int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportTracks";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportTracks: format %d (0 float64, 1 float32)", format); return -1; }
        if (!columns || nColumns <= 0) { set_error("exportTracks: %d columns", nColumns); return -1; }
        if (step_request(what, hop, phase, rowStride) || column_range(what, columns, nColumns, kTrackColumns)) return -1;
        ExportSelection s;
        std::vector<TimelineRow> rows;
        if (step_rows(b, what, utterances, nUtterances, hop, phase, s, rows)) return -1;
        const long long elements = export_elements(what, kStepNouns, s, rowStride, nColumns);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        const bool packed = rowStride == 0, needPitch = std::find(columns, columns + nColumns, 0) != columns + nColumns && s.most > 0;
        const long long pitchStride = needPitch ? s.most : 0;
        std::vector<TimelineList> lists;      // of all pieces, one after the other
        std::vector<ExportPiece> pieces{ExportPiece{0, s.n, 0, {0, 0}}};
        if (needPitch)
            pieces = list_pieces(s.n, [&](long long i) { return b->uttList[(size_t)(utterances ? utterances[i] : i)]; }, [](long long) { return false; }, b->nLists,
                                 std::max<long long>(1, (b->pitchBudgetMB << 20) / (s.most * (long long)sizeof(double))), [&](long long i, uint32_t slot, bool fresh) {
                                     rows[(size_t)i].slot = slot;
                                     if (fresh) lists.push_back(TimelineList{rows[(size_t)i].frame0, (long long)rows[(size_t)i].nFrames});
                                 });
        std::vector<long long> words;      // step starts and chunk rows of all pieces
        long long mostLists = 0;
        for (ExportPiece& pc : pieces) {
            if (packed) pc.table = packed_row_table(s.counts.data(), pc.r0, pc.r1, kTimelineChunkLog2, words);
            mostLists = std::max(mostLists, pc.nLists);
        }
        StageBlock block;
        const int colsAt = block.add(columns, (size_t)nColumns * sizeof(int)), rowsAt = block.add(rows), wordsAt = block.add(words), listsAt = block.add(lists);
        ExportStage stage(b, st, block, needPitch ? &b->pitchOrder : nullptr);
        if (stage.begin([&] { return needPitch ? grow_table(b, b->dPitch, (size_t)(mostLists * pitchStride)) : 0; })) return -1;
        const TimelineRow* dRows = stage.device<TimelineRow>(rowsAt);
        const TimelineList* dLists = stage.device<TimelineList>(listsAt);
        const auto dense = format ? klatt_timeline_dense<true> : klatt_timeline_dense<false>;
        long long elementAt = 0;
        for (const ExportPiece& pc : pieces) {
            const long long nr = pc.r1 - pc.r0;
            const long long pieceElements = (packed ? words[(size_t)(pc.table.startOff + nr)] : nr * rowStride) * nColumns;
            if (pc.nLists > 0) {
                hipLaunchKernelGGL(klatt_timeline_pitch, dim3((unsigned)((pc.nLists + 63) / 64)), dim3(64), 0, st, b->dFrames.ptr, b->dMeta.ptr,
                                   dLists, pc.nLists, hop, phase, pitchStride, b->dPitch.ptr);
                HIP_TRY(hipGetLastError());
                dLists += pc.nLists;
            }
            if (pieceElements > 0) {
                const DenseLaunch d = dense_launch(b, deviceOut, elementAt, pieceElements, elSize, stage.device<long long>(wordsAt), packed ? &pc.table : nullptr);
                hipLaunchKernelGGL(dense, dim3(d.grid), dim3(256), 0, st, b->dFrames.ptr, b->dTimeline.ptr, dRows + pc.r0, d.start, d.chunk, nr, rowStride,
                                   stage.device<int>(colsAt), nColumns, hop, phase, b->dPitch.ptr, pitchStride, (void*)d.out, pieceElements, d.vec);
                HIP_TRY(hipGetLastError());
                elementAt += pieceElements;
            }
        }
        if (stage.finish()) return -1;
        return elements;
    });
}

// ---- phoneme alignment (klatt_align.h) ----------------------------------------------------------------------------------------------
// The rows of an alignment export: count = steps (kind 0), units (1) or frames (2) of every chosen utterance.  0, or -1 with the message set.
static int align_rows(Batch* b, const char* what, const long long* utterances, long long nUtterances, int kind, long long hop, long long phase,
                      ExportSelection& s, std::vector<AlignRow>& rows)
{
    if (!b->hasLabels) { set_error("%s: the batch has no labels (set it with setIpa, setIpaVoices, setText or setRecordsLabelled)", what); return -1; }
    return export_selection(b, what, utterances, nUtterances, true, s, [&](long long, long long u, long long) {
        const long long L = b->lens[(size_t)u];
        const uint32_t l = b->uttList[(size_t)u];
        AlignRow r;
        r.frame0 = b->uttFrameStart[(size_t)u]; r.unit0 = r.frame0 + (long long)l;
        r.nFrames = b->uttFrames[(size_t)u]; r.nUnits = b->listUnits[l]; r.length = (uint32_t)L; r.pad = 0;
        r.count = kind == 0 ? align_steps_below(L, hop, phase) : kind == 1 ? (long long)r.nUnits : (long long)r.nFrames;
        rows.push_back(r);
        return r.count;
    });
}

long long speechPlayer_batch_unitCounts(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int byFrame, long long* counts)
{
    return batch_entry("unitCounts", batch, [&](Batch* b) -> long long {
        ExportSelection s;
        std::vector<AlignRow> rows;
        if (align_rows(b, "unitCounts", utterances, nUtterances, byFrame ? 2 : 1, 1, 0, s, rows)) return -1;
        if (counts) std::copy(s.counts.begin(), s.counts.end(), counts);
        return s.n;
    });
}

// Framewise labels of chosen utterances.  The staging block: columns | rows | step starts and chunk rows (packed).
long long speechPlayer_batch_exportAlignment(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const int* columns,
                                             int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride,
                                             long long pad, long long capacity, void* stream)
{
    const char* what = "exportAlignment";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportAlignment: format %d (0 int64, 1 int32)", format); return -1; }
        if (!columns || nColumns <= 0) { set_error("exportAlignment: %d columns", nColumns); return -1; }
        if (step_request(what, hop, phase, rowStride) || column_range(what, columns, nColumns, kAlignColumns)) return -1;
        int needSpan = 0;
        for (int q = 0; q < nColumns; ++q) needSpan |= columns[q] == kAlignPosition || columns[q] == kAlignRemaining;
        ExportSelection s;
        std::vector<AlignRow> rows;
        if (align_rows(b, what, utterances, nUtterances, 0, hop, phase, s, rows)) return -1;
        const long long elements = export_elements(what, kStepNouns, s, rowStride, nColumns, capacity);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(int) : sizeof(long long);
        if (export_output(b, what, deviceOut, elements, elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        const bool packed = rowStride == 0;
        std::vector<long long> words;
        const RowTable table = packed ? packed_row_table(s.counts.data(), 0, s.n, kTimelineChunkLog2, words) : RowTable{0, 0};
        StageBlock block;
        const int colsAt = block.add(columns, (size_t)nColumns * sizeof(int)), rowsAt = block.add(rows), wordsAt = block.add(words);
        ExportStage stage(b, st, block);
        if (stage.begin()) return -1;
        const DenseLaunch d = dense_launch(b, deviceOut, 0, elements, elSize, stage.device<long long>(wordsAt), packed ? &table : nullptr);
        hipLaunchKernelGGL(format ? klatt_align_dense<true> : klatt_align_dense<false>, dim3(d.grid), dim3(256), 0, st, b->dTimeline.ptr, b->dLabels.ptr,
                           b->dUnitFirst.ptr, stage.device<AlignRow>(rowsAt), d.start, d.chunk, s.n, rowStride, stage.device<int>(colsAt), nColumns, hop, phase,
                           pad, needSpan, deviceOut, elements, d.vec);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

// The segment table of chosen utterances.  The staging block: rows | entry starts (packed).
long long speechPlayer_batch_exportUnits(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, long long hop, long long phase,
                                         int byFrame, void* deviceOut, long long rowStride, long long pad, long long capacity, void* stream)
{
    const char* what = "exportUnits";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (step_request(what, hop, phase, rowStride)) return -1;
        ExportSelection s;
        std::vector<AlignRow> rows;
        if (align_rows(b, what, utterances, nUtterances, byFrame ? 2 : 1, hop, phase, s, rows)) return -1;
        const long long elements = export_elements(what, kEntryNouns, s, rowStride, kUnitColumns, capacity);
        if (elements <= 0) return elements;
        if (export_output(b, what, deviceOut, elements, sizeof(long long))) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        const bool packed = rowStride == 0;
        std::vector<long long> words;
        if (packed) packed_row_table(s.counts.data(), 0, s.n, -1, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        ExportStage stage(b, st, block);
        if (stage.begin()) return -1;
        const long long entries = elements / kUnitColumns;
        const unsigned grid = (unsigned)std::min<long long>((entries + 255) / 256, 8ll * b->cus);
        hipLaunchKernelGGL(klatt_align_units, dim3(grid), dim3(256), 0, st, b->dTimeline.ptr, b->dLabels.ptr, b->dUnitFirst.ptr, stage.device<AlignRow>(rowsAt),
                           packed ? stage.device<long long>(wordsAt) : nullptr, s.n, rowStride, hop, phase, byFrame ? 1 : 0, pad,
                           static_cast<long long*>(deviceOut), entries);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

// ---- the glottal source (klatt_source.h) ----------------------------------------------------------------------------------------------
// One walk over nLists lists (klatt_source.h): a wavefront per list, or a lane per list where there are enough of them to fill the
// device that way (option "source_lane_lists"; profiles/source_export.txt).
static void launch_source_walk(Batch* b, int what, hipStream_t st, const SourceList* dLists, long long nLists, long long hop, long long phase,
                               long long tableStride, double* table, long long* counts, double* epochs)
{
    const double srF = (double)b->sampleRate, invSr = 1.0 / (double)b->sampleRate;      // (KernelArgs' sampleRateF and invSampleRate)
    if (nLists >= b->sourceLaneLists) {
        const auto fn = what == kSourceColumns ? klatt_source_lanes<kSourceColumns> : what == kSourceCount ? klatt_source_lanes<kSourceCount> : klatt_source_lanes<kSourceEpochs>;
        hipLaunchKernelGGL(fn, dim3((unsigned)((nLists + 63) / 64)), dim3(64), 0, st, b->dFrames.ptr, b->dMeta.ptr, b->dTimeline.ptr,
                           dLists, nLists, srF, invSr, hop, phase, tableStride, table, counts, epochs);
    } else {
        const auto fn = what == kSourceColumns ? klatt_source_walk<kSourceColumns> : what == kSourceCount ? klatt_source_walk<kSourceCount> : klatt_source_walk<kSourceEpochs>;
        hipLaunchKernelGGL(fn, dim3((unsigned)nLists), dim3(64), 0, st, b->dFrames.ptr, b->dMeta.ptr, b->dTimeline.ptr,
                           dLists, srF, invSr, hop, phase, tableStride, table, counts, epochs);
    }
}

static SourceList source_list(const Batch* b, long long u, long long out, long long cap)
{
    return SourceList{b->uttFrameStart[(size_t)u], (long long)b->uttFrames[(size_t)u], (long long)b->lens[(size_t)u], out, cap};
}

// The source columns of chosen utterances.  Every export walks the distinct lists its rows speak (those with steps) into the step table,
// in pieces of rows whose lists fit option "source_table_mb", and klatt_source_dense deals the table out to the rows.  The staging
// block: columns | rows | per piece: step starts and chunk rows (packed) | lists.
long long speechPlayer_batch_exportSource(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const int* columns,
                                          int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportSource";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportSource: format %d (0 float64, 1 float32)", format); return -1; }
        if (!columns || nColumns <= 0) { set_error("exportSource: %d columns", nColumns); return -1; }
        if (step_request(what, hop, phase, rowStride) || column_range(what, columns, nColumns, kSourceCols)) return -1;
        ExportSelection s;
        std::vector<TimelineRow> rows;
        if (step_rows(b, what, utterances, nUtterances, hop, phase, s, rows)) return -1;
        const long long elements = export_elements(what, kStepNouns, s, rowStride, nColumns);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        const bool packed = rowStride == 0;
        const long long tableStride = std::max<long long>(s.most, 1);
        std::vector<SourceList> lists;      // of all pieces, one after the other
        std::vector<ExportPiece> pieces =
            list_pieces(s.n, [&](long long i) { return b->uttList[(size_t)(utterances ? utterances[i] : i)]; }, [&](long long i) { return rows[(size_t)i].steps == 0; },
                        b->nLists, std::max<long long>(1, (b->sourceBudgetMB << 20) / (tableStride * kSourceCols * (long long)sizeof(double))),
                        [&](long long i, uint32_t slot, bool fresh) {
                            rows[(size_t)i].slot = slot;
                            if (fresh) lists.push_back(source_list(b, utterances ? utterances[i] : i, 0, 0));
                        });
        std::vector<long long> words;
        long long mostLists = 0;
        for (ExportPiece& pc : pieces) {
            if (packed) pc.table = packed_row_table(s.counts.data(), pc.r0, pc.r1, kTimelineChunkLog2, words);
            mostLists = std::max(mostLists, pc.nLists);
        }
        StageBlock block;
        const int colsAt = block.add(columns, (size_t)nColumns * sizeof(int)), rowsAt = block.add(rows), wordsAt = block.add(words), listsAt = block.add(lists);
        ExportStage stage(b, st, block, &b->sourceOrder);
        if (stage.begin([&] { return grow_table(b, b->dSource, (size_t)(mostLists * tableStride) * kSourceCols); })) return -1;
        const TimelineRow* dRows = stage.device<TimelineRow>(rowsAt);
        const SourceList* dLists = stage.device<SourceList>(listsAt);
        const auto dense = format ? klatt_source_dense<true> : klatt_source_dense<false>;
        long long elementAt = 0;
        for (const ExportPiece& pc : pieces) {
            const long long nr = pc.r1 - pc.r0;
            const long long pieceElements = (packed ? words[(size_t)(pc.table.startOff + nr)] : nr * rowStride) * nColumns;
            if (pc.nLists > 0) {
                launch_source_walk(b, kSourceColumns, st, dLists, pc.nLists, hop, phase, tableStride, b->dSource.ptr, nullptr, nullptr);
                HIP_TRY(hipGetLastError());
                dLists += pc.nLists;
            }
            if (pieceElements > 0) {
                const DenseLaunch d = dense_launch(b, deviceOut, elementAt, pieceElements, elSize, stage.device<long long>(wordsAt), packed ? &pc.table : nullptr);
                hipLaunchKernelGGL(dense, dim3(d.grid), dim3(256), 0, st, b->dSource.ptr, tableStride, dRows + pc.r0, d.start, d.chunk, nr, rowStride,
                                   stage.device<int>(colsAt), nColumns, (void*)d.out, pieceElements, d.vec);
                HIP_TRY(hipGetLastError());
                elementAt += pieceElements;
            }
        }
        if (stage.finish()) return -1;
        return elements;
    });
}

// The epochs of every list of the batch as set: one counting walk on the batch's own stream, downloaded, kept until the next set call.
static int epoch_counts(Batch* b)
{
    if (b->epochFresh) return 0;
    if (b->nFrames >= 0xFFFFFFFFll || b->nLists > 0x7FFFFFFFll) { set_error("epochCounts: too many frames"); return -1; }
    b->epochCount.assign((size_t)b->nLists, 0);
    if (b->nLists == 0) { b->epochFresh = true; return 0; }
    HIP_TRY(hipSetDevice(b->device));
    std::vector<SourceList> lists((size_t)b->nLists, SourceList{0, 0, 0, 0, 0});      // (a list no utterance speaks has no samples)
    for (long long u = 0; u < b->nUtt; ++u) lists[b->uttList[(size_t)u]] = source_list(b, u, 0, 0);
    StageBlock block;
    const int listsAt = block.add(lists);
    ExportStage stage(b, b->stream, block);
    if (stage.begin([&] { return grow_table(b, b->dEpochCount, (size_t)b->nLists); })) return -1;
    launch_source_walk(b, kSourceCount, b->stream, stage.device<SourceList>(listsAt), b->nLists, 1, 0, 0, nullptr, b->dEpochCount.ptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->epochCount.data(), b->dEpochCount.ptr, (size_t)b->nLists * sizeof(long long), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));      // (the host has waited: the slot is free again without an event)
    b->epochFresh = true;
    return 0;
}

long long speechPlayer_batch_epochCounts(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, long long* counts)
{
    return batch_entry("epochCounts", batch, [&](Batch* b) -> long long {
        const long long n = check_selection(b, "epochCounts", utterances, nUtterances, false);
        if (n < 0 || epoch_counts(b)) return -1;
        for (long long i = 0; counts && i < n; ++i) counts[i] = b->epochCount[b->uttList[(size_t)(utterances ? utterances[i] : i)]];
        return n;
    });
}

// The epoch table of chosen utterances.  The counts come from epoch_counts (the first call after a set call waits for the counting walk);
// the writing walk takes the distinct lists with epochs that the rows speak, and klatt_source_deal copies their tables to the rows.
// The staging block: rows | entry starts (packed) | lists.
long long speechPlayer_batch_exportEpochs(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, void* deviceOut,
                                          long long rowStride, double pad, long long capacity, void* stream)
{
    const char* what = "exportEpochs";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (rowStride < 0) { set_error("exportEpochs: rowStride %lld", rowStride); return -1; }
        if (check_selection(b, what, utterances, nUtterances, false) < 0 || epoch_counts(b)) return -1;      // (refusals before the device)
        std::vector<EpochRow> rows;
        std::vector<SourceList> lists;
        std::vector<long long> slotOf((size_t)b->nLists, -1);
        long long tableEntries = 0;
        ExportSelection s;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long, long long u, long long) {
                const uint32_t l = b->uttList[(size_t)u];
                const long long count = b->epochCount[l];
                if (count > 0 && slotOf[l] < 0) {
                    slotOf[l] = (long long)lists.size();
                    lists.push_back(source_list(b, u, tableEntries, count));
                    tableEntries += count;
                }
                rows.push_back(EpochRow{count > 0 ? lists[(size_t)slotOf[l]].out : 0, count});
                return count;
            })) return -1;
        const long long elements = export_elements(what, kEntryNouns, s, rowStride, kEpochCols, capacity);
        if (elements <= 0) return elements;
        if (export_output(b, what, deviceOut, elements, sizeof(double))) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        const bool packed = rowStride == 0;
        std::vector<long long> words;
        if (packed) packed_row_table(s.counts.data(), 0, s.n, -1, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), listsAt = block.add(lists);
        ExportStage stage(b, st, block, &b->sourceOrder);
        if (stage.begin([&] { return grow_table(b, b->dEpochs, (size_t)tableEntries * kEpochCols); })) return -1;
        if (!lists.empty()) {
            launch_source_walk(b, kSourceEpochs, st, stage.device<SourceList>(listsAt), (long long)lists.size(), 1, 0, 0, nullptr, nullptr, b->dEpochs.ptr);
            HIP_TRY(hipGetLastError());
        }
        const long long entries = elements / kEpochCols;
        const unsigned grid = (unsigned)std::min<long long>((entries + 255) / 256, 8ll * b->cus);
        hipLaunchKernelGGL(klatt_source_deal, dim3(grid), dim3(256), 0, st, b->dEpochs.ptr, stage.device<EpochRow>(rowsAt),
                           packed ? stage.device<long long>(wordsAt) : nullptr, s.n, rowStride, pad, static_cast<double*>(deviceOut), entries,
                           reinterpret_cast<uintptr_t>(deviceOut) % 16 == 0 ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

// ---- vocal-tract frequency response (klatt_response.h) ---------------------------------------------------------------------------------
// The arguments both entry points share.  0, or -1 with the message set.
static int response_request(const char* what, const double* frequencies, int nFrequencies, const int* kinds, int nKinds)
{
    if (nFrequencies < 1 || nFrequencies > kRespMaxBins) { set_error("%s: %d frequencies (1 .. %d)", what, nFrequencies, kRespMaxBins); return -1; }
    if (!frequencies) { set_error("%s: no frequencies", what); return -1; }
    for (int k = 0; k < nFrequencies; ++k)
        if (!std::isfinite(frequencies[k])) { set_error("%s: frequencies[%d] is not finite", what, k); return -1; }
    if (!kinds || nKinds <= 0) { set_error("%s: %d kinds", what, nKinds); return -1; }
    for (int q = 0; q < nKinds; ++q)
        if (kinds[q] < 0 || kinds[q] >= kRespKinds) { set_error("%s: kinds[%d] = %d (0 .. %d)", what, q, kinds[q], kRespKinds - 1); return -1; }
    return 0;
}

// Host only, touches no device: the definition of include/speechPlayer_batch.h on plain frames, out[frame][kind][bin], through the
// functions the kernel is compiled from (klatt_response.h).
long long speechPlayer_frameResponse(const speechPlayer_frame_t* frames, long long nFrames, int sampleRate, const double* frequencies,
                                     int nFrequencies, const int* kinds, int nKinds, int gain, double* out)
{
    begin_call();
    if (nFrames < 0 || sampleRate <= 0 || (nFrames > 0 && (!frames || !out))) { set_error("frameResponse: bad arguments"); return -1; }
    if (response_request("frameResponse", frequencies, nFrequencies, kinds, nKinds)) return -1;
    try {
        std::vector<double> tw((size_t)nFrequencies * 4);
        for (int k = 0; k < nFrequencies; ++k) response_twiddles(frequencies[k], sampleRate, tw.data() + (size_t)k * 4);
        bool needC = false, needP = false;
        for (int q = 0; q < nKinds; ++q) { needC = needC || kinds[q] < 4; needP = needP || kinds[q] >= 4; }
        const KernelArgs a = base_args(sampleRate);
        const double* f = reinterpret_cast<const double*>(frames);
        double V[kRespVals];
        for (long long i = 0; i < nFrames; ++i) {
            response_values_host(f + i * kNumParams, a.negPiOverSr, a.twoPiOverSr, V);
            double* o = out + (size_t)i * nKinds * nFrequencies;
            for (int k = 0; k < nFrequencies; ++k) {
                Cx C, P;
                const double* w = tw.data() + (size_t)k * 4;
                response_bin(V, w[0], w[1], w[2], w[3], gain != 0, needC, needP, C, P);
                for (int q = 0; q < nKinds; ++q) o[(size_t)q * nFrequencies + k] = response_kind(kinds[q], C, P);
            }
        }
    } catch (const std::exception& e) { set_error("frameResponse: %s", e.what()); return -1; }
    return nFrames * nKinds * nFrequencies;
}

// The response of chosen utterances (one piece: no table).  Rows that speak one frame list form a group, computed once and stored to each
// of its rows (klatt_response.h).  The twiddles are made here, by the functions speechPlayer_frameResponse uses.  The staging block:
// twiddles | kinds | groups | the rows' first steps, group after group.
long long speechPlayer_batch_exportResponse(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
                                            const double* frequencies, int nFrequencies, const int* kinds, int nKinds, int gain, long long hop,
                                            long long phase, void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportResponse";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportResponse: format %d (0 float64, 1 float32)", format); return -1; }
        if (response_request(what, frequencies, nFrequencies, kinds, nKinds) || step_request(what, hop, phase, rowStride)) return -1;
        const bool packed = rowStride == 0;
        const long long perStep = (long long)nKinds * nFrequencies;
        std::vector<ResponseGroup> groups;
        std::vector<long long> groupOf((size_t)b->nLists, -1), rowGroup, rowFirst;
        ExportSelection s;
        if (export_selection(b, what, utterances, nUtterances, true, s, [&](long long i, long long u, long long before) {
                const uint32_t l = b->uttList[(size_t)u];
                if (groupOf[l] < 0) {
                    ResponseGroup g;
                    g.frame0 = b->uttFrameStart[(size_t)u]; g.nFrames = b->uttFrames[(size_t)u]; g.nRows = 0;
                    g.steps = align_steps_below(b->lens[(size_t)u], hop, phase);
                    g.span = 0; g.chunk0 = 0; g.rowAt = 0;
                    groupOf[l] = (long long)groups.size();
                    groups.push_back(g);
                }
                ResponseGroup& g = groups[(size_t)groupOf[l]];
                if (g.nRows == 0xFFFFFFFFu) { set_error("exportResponse: too many rows of one frame list"); return -1ll; }
                ++g.nRows;
                rowGroup.push_back(groupOf[l]);
                rowFirst.push_back(packed ? before : i * rowStride);
                return (long long)g.steps;
            })) return -1;
        static constexpr ExportNouns kValueNouns{"largest step count", "steps", "values"};
        const long long elements = export_elements(what, kValueNouns, s, rowStride, perStep);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        // the groups that write anything, their chunks one after the other, and their rows' first steps side by side
        std::vector<ResponseGroup> live;
        std::vector<long long> liveOf(groups.size(), -1);
        long long nChunks = 0, rowAt = 0;
        for (size_t g = 0; g < groups.size(); ++g) {
            ResponseGroup G = groups[g];
            G.span = packed ? G.steps : rowStride;
            if (G.span == 0) continue;
            G.chunk0 = nChunks; G.rowAt = rowAt;
            nChunks += (G.span + kRespSteps - 1) / kRespSteps;
            rowAt += G.nRows;
            liveOf[g] = (long long)live.size();
            live.push_back(G);
        }
        std::vector<long long> rowBase((size_t)rowAt), fill(live.size(), 0);
        for (long long i = 0; i < s.n; ++i) {
            const long long g = liveOf[(size_t)rowGroup[(size_t)i]];
            if (g < 0) continue;
            rowBase[(size_t)(live[(size_t)g].rowAt + fill[(size_t)g]++)] = rowFirst[(size_t)i];
        }
        std::vector<double> tw((size_t)nFrequencies * 4);
        for (int k = 0; k < nFrequencies; ++k) response_twiddles(frequencies[k], b->sampleRate, tw.data() + (size_t)k * 4);
        StageBlock block;
        const int twAt = block.add(tw), kindsAt = block.add(kinds, (size_t)nKinds * sizeof(int)), groupsAt = block.add(live), basesAt = block.add(rowBase);
        ExportStage stage(b, st, block);
        if (stage.begin()) return -1;
        const KernelArgs ka = base_args(b->sampleRate);
        ResponseArgs A;
        A.frames = b->dFrames.ptr; A.req = b->dTimeline.ptr;
        A.groups = stage.device<ResponseGroup>(groupsAt); A.nGroups = (long long)live.size(); A.nChunks = nChunks;
        A.rowBase = stage.device<long long>(basesAt);
        A.hop = hop; A.phase = phase;
        A.kinds = stage.device<int>(kindsAt); A.nKinds = nKinds;
        A.tw = stage.device<double>(twAt); A.K = nFrequencies;
        A.gain = gain != 0; A.needC = 0; A.needP = 0;
        for (int q = 0; q < nKinds; ++q) { if (kinds[q] < 4) A.needC = 1; else A.needP = 1; }
        A.negPiOverSr = ka.negPiOverSr; A.twoPiOverSr = ka.twoPiOverSr;
        A.out = deviceOut;
        const unsigned grid = (unsigned)std::min<long long>(nChunks, 16ll * b->cus);
        hipLaunchKernelGGL(format ? klatt_response<true> : klatt_response<false>, dim3(grid), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

// ---- signal stems (klatt_stems.h) -------------------------------------------------------------------------------------------------------
// Host only, touches no device: (a, b, c) of n resonators as the synthesis kernels compute them from (frequency, bandwidth) --
// coefficient_finish(coefficient_parts(..)) through the host's fast_exp / fast_cos (klatt_response.h), abc[n][3].
long long speechPlayer_resonatorCoefficients(const double* frequency, const double* bandwidth, long long n, int anti, int sampleRate, double* abc)
{
    begin_call();
    if (n < 0 || sampleRate <= 0 || (n > 0 && (!frequency || !bandwidth || !abc))) { set_error("resonatorCoefficients: bad arguments"); return -1; }
    const KernelArgs a = base_args(sampleRate);
    for (long long i = 0; i < n; ++i) {
        const Coef k = resonator_coefficients_host(frequency[i], bandwidth[i], anti != 0, a.negPiOverSr, a.twoPiOverSr);
        abc[3 * i] = k.a; abc[3 * i + 1] = k.b; abc[3 * i + 2] = k.c;
    }
    return n;
}

// The stems of chosen utterances (no hop; the output is planar).  One lane per row, the rows sorted by length (klatt_stems.h).  The
// staging block: columns | rows.
long long speechPlayer_batch_exportStems(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const int* columns,
                                         int nColumns, void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportStems";
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("exportStems: format %d (0 float64, 1 float32)", format); return -1; }
        if (!columns || nColumns <= 0) { set_error("exportStems: %d columns", nColumns); return -1; }
        if (rowStride < 0) { set_error("exportStems: rowStride %lld", rowStride); return -1; }
        if (column_range(what, columns, nColumns, kStemColumns)) return -1;
        StemArgs A;
        memset(&A, 0, sizeof A);
        for (int c = 0; c < kStemColumns; ++c) A.slotOf[c] = -1;
        for (int q = 0; q < nColumns; ++q)
            if (A.slotOf[columns[q]] < 0) A.slotOf[columns[q]] = A.nSlots++;
        const bool packed = rowStride == 0;
        ExportSelection s;
        std::vector<StemRow> rows;
        if (export_selection(b, what, utterances, nUtterances, true, s, [&](long long i, long long u, long long before) {
                StemRow r;
                r.frame0 = b->uttFrameStart[(size_t)u]; r.nFrames = b->uttFrames[(size_t)u]; r.seed = b->uttSeed[(size_t)u];
                r.length = b->lens[(size_t)u]; r.pad = 0;
                r.out = packed ? before : i;      // (the samples or rows before the row; elements below)
                rows.push_back(r);
                return (long long)r.length;
            })) return -1;
        static constexpr ExportNouns kSampleNouns{"longest utterance", "samples", "columns"};
        const long long elements = export_elements(what, kSampleNouns, s, rowStride, nColumns);
        if (elements < 0) return -1;
        if (s.n > 0x7FFFFFFFll * kLanes) { set_error("exportStems: %lld rows", s.n); return -1; }
        if (elements == 0) return 0;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        for (StemRow& r : rows) r.out = (packed ? r.out : r.out * rowStride) * nColumns;
        // a wavefront runs as long as its longest lane: the rows longest first (each knows its place in the output)
        std::stable_sort(rows.begin(), rows.end(), [](const StemRow& x, const StemRow& y) { return x.length > y.length; });
        StageBlock block;
        const int colsAt = block.add(columns, (size_t)nColumns * sizeof(int)), rowsAt = block.add(rows);
        const int el = (int)elSize, T = stem_tile(A.nSlots, el), ldsBytes = stem_lds_bytes(A.nSlots, el);
        const auto kernel = format ? klatt_stems<true, 16> : T == 16 ? klatt_stems<false, 16> : klatt_stems<false, 8>;
        ExportStage stage(b, st, block);
        if (stage.begin([&] { return ensure_lds_limit(reinterpret_cast<const void*>(kernel), kStemLdsBudget); })) return -1;
        A.K = base_args(b->sampleRate);
        A.K.frames = b->dFrames.ptr; A.K.meta = b->dMeta.ptr;
        A.rows = stage.device<StemRow>(rowsAt); A.nRows = s.n;
        A.columns = stage.device<int>(colsAt); A.nColumns = nColumns;
        A.rowStride = rowStride; A.out = deviceOut;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((s.n + kLanes - 1) / kLanes)), dim3(kLanes), ldsBytes, st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

// ---- what the spectrogram, resampled, convolved, mixed and power exports read ----------------------------------------------------------------------------
// The batch's pool, a row per utterance (sig null), or a caller's signal (speechPlayer_signal_t; klatt_tiles.h: signal_plan, the reader).
// An entry point over a signal differs from its sibling over the pool in four places, all here (export_input decides): the rows it may choose
// (export_selection's `sig`), no synthesis is needed (export_synthesised is skipped), the signal's memory is checked beside the output's
// (signal_memory) and the stage is ExportStage's ofSignal.
static_assert(sizeof(speechPlayer_signal_t) == 40 && offsetof(speechPlayer_signal_t, extent) == 32, "speechPlayer_signal_t is five 8-byte words");
struct ExportInput {
    Batch* b;
    const SignalPlan* sig = nullptr;
    const void* data = nullptr;          // the pool, or the signal's data
    long long at(long long r) const { return sig ? sig->at(r) : b->outStart[(size_t)r]; }
    long long len(long long r) const { return sig ? sig->len(r) : (long long)b->lens[(size_t)r]; }
    long long rows() const { return sig ? sig->nRows : b->nUtt; }
    int format() const { return sig ? sig->format : 0; }
};
// What an entry point reads: the pool (ofSignal false; `signal` is not looked at), or `signal` with the refusals that need no device, in
// the header's order
static int export_input(Batch* b, const char* what, bool ofSignal, const speechPlayer_signal_t* signal, SignalPlan& P, ExportInput& in)
{
    if (!ofSignal) { in = ExportInput{b, nullptr, b->dPcm.ptr}; return 0; }
    if (!signal) { set_error("%s: no signal", what); return -1; }
    std::string why;
    if (!signal_plan(P, signal->format, signal->nRows, signal->rowStride, signal->extent, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
    in = ExportInput{b, &P, signal->data};
    return 0;
}
// ... and those of its memory, once the output's are past: device memory of the batch's device that holds every row, aligned to its
// element, apart from the output.  A signal whose rows are all empty is never read and may have no data.
static int signal_memory(const ExportInput& in, const char* what, const void* deviceOut, size_t outBytes)
{
    if (!in.sig || in.sig->need == 0) return 0;
    const size_t bytes = (size_t)in.sig->need * (size_t)in.sig->elSize;
    if (!in.data) { set_error("%s: signal without data", what); return -1; }
    const std::string name = std::string(what) + ": signal";
    if (!device_range(in.data, bytes, in.b->device, (size_t)in.sig->elSize, name.c_str())) return -1;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in.data), o = reinterpret_cast<uintptr_t>(deviceOut);
    if (a < o + outBytes && o < a + bytes) { set_error("%s: the output (%zu bytes from %p) overlaps the signal (%zu bytes from %p)", what, outBytes, deviceOut, bytes, in.data); return -1; }
    return 0;
}

// ---- STFT and band spectrogram of the PCM (klatt_spectrum.h) -----------------------------------------------------------------------------
// Host only, touches no device: the definition of include/speechPlayer_batch.h on plain PCM, out[step][band], through the functions the
// kernel is compiled from (klatt_spectrum.h).
// The host statements over a signal's samples (speechPlayer_signal*): the input format, first of their refusals, and the values of
// float32 samples, last of them (once there is something to compute)
static int signal_host_format(const char* what, int inFormat)
{
    if (inFormat != 0 && inFormat != 1) { set_error("%s: input format %d (0 int16, 1 float32)", what, inFormat); return -1; }
    return 0;
}
static int signal_host_values(const char* what, const void* x, int inFormat, long long length)
{
    std::string why;
    if (inFormat == 1 && length > 0 && x && !signal_values(static_cast<const float*>(x), length, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
    return 0;
}

static long long spectrogram_statement(const char* what, const void* x, int inFormat, long long length, int nFft, long long hop, long long phase, const double* window,
                                       const double* bank, int nBands, int power, double logScale, double floor, double* out)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || hop <= 0 || phase < 0 || (length > 0 && !x)) { set_error("%s: length %lld, hop %lld, phase %lld", what, length, hop, phase); return -1; }
    try {
        SpecPlan P;
        std::string why;
        if (!spec_plan(P, nFft, window, bank, nBands, power, logScale, floor, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
        if (align_steps_below(length, hop, phase) > 0 && !out) { set_error("%s: no output", what); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? spectrogram_host(static_cast<const float*>(x), length, P, hop, phase, out)
                        : spectrogram_host(static_cast<const int16_t*>(x), length, P, hop, phase, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmSpectrogram(const sample* pcm, long long length, int nFft, long long hop, long long phase, const double* window,
                                      const double* bank, int nBands, int power, double logScale, double floor, double* out)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return spectrogram_statement("pcmSpectrogram", pcm, 0, length, nFft, hop, phase, window, bank, nBands, power, logScale, floor, out);
}

long long speechPlayer_signalSpectrogram(const void* x, int inFormat, long long length, int nFft, long long hop, long long phase, const double* window,
                                         const double* bank, int nBands, int power, double logScale, double floor, double* out)
{
    begin_call();
    return spectrogram_statement("signalSpectrogram", x, inFormat, length, nFft, hop, phase, window, bank, nBands, power, logScale, floor, out);
}

// What a spectrogram kernel takes of the plan, the step grid, the packed form's row table (null: padded) and the output: everything but
// the input, the rows and the plan's arrays on the device (the whole-row export's and the stage's: klatt_stage_window.h)
static SpecArgs spec_args(const ExportStage& stage, const SpecPlan& P, const RowTable* table, int wordsAt, long long rowStride, long long elements, long long hop,
                          long long phase, void* deviceOut)
{
    SpecArgs A{};
    A.start = table ? stage.device<long long>(wordsAt) + table->startOff : nullptr;
    A.chunk = table ? stage.device<long long>(wordsAt) + table->chunkOff : nullptr;
    A.rowStride = rowStride; A.nSteps = elements / P.nOut;
    A.hop = hop; A.phase = phase;
    A.logN = P.logN; A.nOut = P.nOut; A.hasBank = P.hasBank; A.power = P.power;
    A.logScale = P.logScale; A.floor = P.floor;
    A.out = deviceOut; A.vec = reinterpret_cast<uintptr_t>(deviceOut) % 16 == 0;
    return A;
}
// A spectrogram kernel over the steps of `S`, four a workgroup, queued on the stage's stream
extern "C++" template <class Args>
static int queue_spectrogram(const ExportStage& stage, void (*kernel)(Args), const Args& A, const SpecArgs& S)
{
    const long long nGroups = (S.nSteps + kSpecWaves - 1) / kSpecWaves;
    const unsigned grid = (unsigned)std::min<long long>(nGroups, 16ll * stage.b->cus);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kSpecWaves), (size_t)kSpecWaves * spec_lds_wave(1 << (S.logN - 1)), stage.st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The spectrogram of chosen utterances' PCM, one wavefront per step (klatt_spectrum.h).  It reads the pool, so it is ordered as
// speechPlayer_batch_exportPcm is (ExportStage, ofPcm).  The staging block: rows | step starts and chunk rows (packed) | window |
// twiddles | band weights | band ranges.
// ofSignal: the rows are chosen from and read from `signal` in place of the pool (export_input).
static long long spectrogram_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances, int nFft,
                                    long long hop, long long phase, const double* window, const double* bank, int nBands, int power,
                                    double logScale, double floor, void* deviceOut, int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("%s: format %d (0 float64, 1 float32)", what, format); return -1; }
        if (step_request(what, hop, phase, rowStride)) return -1;
        SpecPlan P;
        std::string why;
        if (!spec_plan(P, nFft, window, bank, nBands, power, logScale, floor, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<SpecRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long, long long u, long long) {
                const long long L = in.len(u);
                rows.push_back(SpecRow{in.at(u), L, align_steps_below(L, hop, phase)});
                return rows.back().steps;
            }, in.sig)) return -1;
        static constexpr ExportNouns kBandNouns{"largest step count", "steps", "bands"};
        const long long elements = export_elements(what, kBandNouns, s, rowStride, P.nOut);
        if (elements <= 0) return elements;
        if (!in.sig && export_synthesised(b, what)) return -1;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize) || signal_memory(in, what, deviceOut, (size_t)elements * elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        const bool packed = rowStride == 0;
        std::vector<long long> words;
        const RowTable table = packed ? packed_row_table(s.counts.data(), 0, s.n, kTimelineChunkLog2, words) : RowTable{0, 0};
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), windowAt = block.add(P.window), twAt = block.add(P.tw),
                  weightsAt = block.add(P.weights), rangeAt = block.add(P.range);
        // the kernel of the input's and the output's type
        void (*const kernels[2][2])(SpecArgs) = {{klatt_spectrogram<false, int16_t>, klatt_spectrogram<true, int16_t>}, {klatt_spectrogram<false, float>, klatt_spectrogram<true, float>}};
        const auto kernel = kernels[in.format()][format];
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin([&] { return ensure_lds_limit(reinterpret_cast<const void*>(kernel), kSpecLdsBudget); })) return -1;
        SpecArgs A = spec_args(stage, P, packed ? &table : nullptr, wordsAt, rowStride, elements, hop, phase, deviceOut);
        A.in = in.data; A.rows = stage.device<SpecRow>(rowsAt);
        A.window = stage.device<float>(windowAt); A.tw = stage.device<SpecCx>(twAt);
        A.weights = stage.device<float>(weightsAt); A.range = stage.device<int>(rangeAt);
        if (queue_spectrogram(stage, kernel, A, A) || stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportSpectrogram(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int nFft,
                                               long long hop, long long phase, const double* window, const double* bank, int nBands, int power,
                                               double logScale, double floor, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportSpectrogram")) return -1;
    return spectrogram_export("exportSpectrogram", batch, false, nullptr, utterances, nUtterances,
                              nFft, hop, phase, window, bank, nBands, power, logScale, floor, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportSpectrogramOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int nFft,
                                                 long long hop, long long phase, const double* window, const double* bank, int nBands, int power,
                                                 double logScale, double floor, void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportSpectrogramOf";
    if (refuse_timing_only("speechPlayer_batch_exportSpectrogramOf")) return -1;
    return spectrogram_export(what, batch, true, signal, rows, nRows,
                              nFft, hop, phase, window, bank, nBands, power, logScale, floor, deviceOut, format, rowStride, stream);
}

// ---- the tile-wise exports of the PCM (klatt_tiles.h): resampled, convolved, mixed ---------------------------------------------------------
// A workgroup takes tiles of one row: the packed form's row table counts TILES (klatt_export.h: tile_row_table), the rows carry their
// first element in the output.  An entry point is, in the order of its refusals: tile_request, its own plan, export_selection with
// tile_row_first, tile_elements, ExportStage with the words of tile_row_table, its own launches, tile_out and launch_tiles (which finishes).
constexpr ExportNouns kSampleNouns{"longest output row", "samples", nullptr};
static int tile_request(const char* what, int format, long long rowStride)
{
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    if (rowStride < 0) { set_error("%s: rowStride %lld", what, rowStride); return -1; }
    return 0;
}
// Row i's first element in the output: i rows of rowStride (padded: export_elements refuses an extent that wraps) or the outputs before it
static long long tile_row_first(long long i, long long rowStride, long long before) { return rowStride > 0 ? (long long)((unsigned long long)i * (unsigned long long)rowStride) : before; }
// The elements of the export (0: nothing to do), or -1 with the message set: the extent, a batch not synthesised, the output, in this order
// (an export of a signal needs no synthesis; its memory is checked beside the output's)
static long long tile_elements(Batch* b, const char* what, const ExportSelection& s, long long rowStride, int format, void* deviceOut, const ExportInput* in = nullptr)
{
    const long long elements = export_elements(what, kSampleNouns, s, rowStride, 1);
    if (elements <= 0) return elements;
    const size_t elSize = format ? sizeof(float) : sizeof(int16_t);
    if (!(in && in->sig) && export_synthesised(b, what)) return -1;
    if (export_output(b, what, deviceOut, elements, elSize) || (in && signal_memory(*in, what, deviceOut, (size_t)elements * elSize))) return -1;
    return elements;
}
static TileOut tile_out(const ExportStage& stage, int wordsAt, const TileTable& t, long long rowStride, void* deviceOut)
{
    const long long* words = rowStride == 0 ? stage.device<long long>(wordsAt) : nullptr;      // (the padded form has no row table)
    return TileOut{words ? words + t.table.startOff : nullptr, words ? words + t.table.chunkOff : nullptr, rowStride, t.tilesPerRow, t.nTiles, deviceOut};
}
// The kernel of the format over the tiles, at most perCu workgroups per CU, queued on the stage's stream
extern "C++" template <class Args>
static int queue_tiles(const ExportStage& stage, void (*int16)(Args), void (*float32)(Args), int format, long long perCu, const Args& A)
{
    const unsigned grid = (unsigned)std::min<long long>(A.tile.nTiles, perCu * stage.b->cus);
    hipLaunchKernelGGL(format ? float32 : int16, dim3(grid), dim3(256), 0, stage.st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ... as the stage's last launch
extern "C++" template <class Args>
static int launch_tiles(ExportStage& stage, void (*int16)(Args), void (*float32)(Args), int format, long long perCu, const Args& A)
{
    return queue_tiles(stage, int16, float32, format, perCu, A) || stage.finish() ? -1 : 0;
}

// The same with a kernel per input type: kernels[input format][output format]
extern "C++" template <class Args>
static int launch_tiles(ExportStage& stage, void (*const (&kernels)[2][2])(Args), int inFormat, int format, long long perCu, const Args& A)
{
    return launch_tiles(stage, kernels[inFormat][0], kernels[inFormat][1], format, perCu, A);
}

// ---- the PCM at another sample rate (klatt_resample.h) -----------------------------------------------------------------------------------
// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernel is compiled from.
long long speechPlayer_resampledLength(long long length, int srcRate, int dstRate)
{
    begin_call();
    if (length < 0 || srcRate <= 0 || dstRate <= 0) { set_error("resampledLength: length %lld, %d to %d Hz", length, srcRate, dstRate); return -1; }
    const long long g = res_gcd(srcRate, dstRate);
    return res_length(length, dstRate / g, srcRate / g);
}

long long speechPlayer_resampleKernel(int srcRate, int dstRate, int zeros, double rolloff, int window, double beta, int* up, int* down, int* taps,
                                      double* table, long long capacity)
{
    begin_call();
    try {
        ResPlan P;
        std::string why;
        if (!res_plan(P, srcRate, dstRate, zeros, rolloff, window, beta, why)) { set_error("resampleKernel: %s", why.c_str()); return -1; }
        const long long n = (long long)P.table.size();
        if (table && capacity < n) { set_error("resampleKernel: the table takes %lld values, capacity is %lld", n, capacity); return -1; }
        if (up) *up = P.up;
        if (down) *down = P.down;
        if (taps) *taps = P.taps;
        for (long long i = 0; table && i < n; ++i) table[i] = (double)P.table[(size_t)i];
        return n;
    } catch (const std::exception& e) { set_error("resampleKernel: %s", e.what()); return -1; }
}

static long long resample_statement(const char* what, const void* x, int inFormat, long long length, int srcRate, int dstRate, int zeros, double rolloff, int window,
                                    double beta, int format, void* out, long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || (length > 0 && !x)) { set_error("%s: length %lld (0 .. 2^44, with its samples)", what, length); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    try {
        ResPlan P;
        std::string why;
        if (!res_plan(P, srcRate, dstRate, zeros, rolloff, window, beta, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        const long long Lout = res_length(length, P.up, P.down);
        if (!out) return Lout;
        if (capacity < Lout) { set_error("%s: the output takes %lld elements, capacity is %lld", what, Lout, capacity); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? resample_host(static_cast<const float*>(x), length, P, format, out) : resample_host(static_cast<const int16_t*>(x), length, P, format, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmResample(const sample* pcm, long long length, int srcRate, int dstRate, int zeros, double rolloff, int window, double beta,
                                   int format, void* out, long long capacity)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return resample_statement("pcmResample", pcm, 0, length, srcRate, dstRate, zeros, rolloff, window, beta, format, out, capacity);
}

long long speechPlayer_signalResample(const void* x, int inFormat, long long length, int srcRate, int dstRate, int zeros, double rolloff, int window, double beta,
                                      int format, void* out, long long capacity)
{
    begin_call();
    return resample_statement("signalResample", x, inFormat, length, srcRate, dstRate, zeros, rolloff, window, beta, format, out, capacity);
}

// Equal rates of a signal: klatt_signal_copy (input format, output format) over the tiles, on the stage's stream -- no table, no filter
static int launch_signal_copy(const ExportStage& stage, const ExportInput& in, int format, const ResRow* rows, const TileOut& tile)
{
    ResArgs A;
    A.in = in.data; A.rows = rows; A.tile = tile;
    A.hT = nullptr; A.up = A.down = 1; A.Z = 0; A.span = kResampleTile;
    void (*const copies[2][2])(ResArgs) = {{klatt_signal_copy<false, int16_t>, klatt_signal_copy<true, int16_t>}, {klatt_signal_copy<false, float>, klatt_signal_copy<true, float>}};
    const unsigned grid = (unsigned)std::min<long long>(tile.nTiles, 8ll * stage.b->cus);
    hipLaunchKernelGGL(copies[in.format()][format], dim3(grid), dim3(256), 0, stage.st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The chosen utterances' PCM at `outRate` (klatt_resample.h).  It reads the pool, so it is ordered as speechPlayer_batch_exportPcm is
// (ExportStage, ofPcm), tile-wise.  The staging block: rows | tile starts and chunk rows (packed) | the table, when the batch does not hold it.
// The table stays on the batch until the parameters change; the exports that read it follow one order (resampleOrder).
// ofSignal and `signal` as spectrogram_export's; over the pool srcRate is the batch's rate.  Equal rates: -2 over the pool (the caller answers with
// speechPlayer_batch_exportPcm), the copy kernel over a signal.
static long long resampled_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances, int srcRate,
                                  int outRate, int zeros, double rolloff, int window, double beta, void* deviceOut, int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        if (!in.sig) srcRate = b->sampleRate;
        if (!b->resPlan.same(srcRate, outRate, zeros, rolloff, window, beta)) {
            ResPlan P;
            std::string why;
            if (!res_plan(P, srcRate, outRate, zeros, rolloff, window, beta, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
            b->resPlan = std::move(P);
            b->resOnDevice = false;
        }
        ResPlan& P = b->resPlan;
        if (P.identity && !in.sig) return -2;      // equal rates: speechPlayer_batch_exportPcm's output exactly
        ExportSelection s;
        std::vector<ResRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) {
                const long long L = in.len(u), Lout = res_length(L, P.up, P.down);
                rows.push_back(ResRow{in.at(u), L, Lout, tile_row_first(i, rowStride, before)});
                return Lout;
            }, in.sig)) return -1;
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        hipStream_t st = static_cast<hipStream_t>(stream);

        std::vector<long long> words;
        const TileTable tiles = tile_row_table(s.counts.data(), s.n, kResampleTile, rowStride, kTimelineChunkLog2, words);
        if (P.identity) {      // a signal at its own rate: no table, no filter
            StageBlock block;
            const int rowsAt = block.add(rows), wordsAt = block.add(words);
            ExportStage stage(b, st, block, nullptr, false, true);
            if (stage.begin()) return -1;
            if (launch_signal_copy(stage, in, format, stage.device<ResRow>(rowsAt), tile_out(stage, wordsAt, tiles, rowStride, deviceOut)) || stage.finish()) return -1;
            return elements;
        }
        const bool upload = !b->resOnDevice;
        if (upload) res_transpose(P);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), tableAt = upload ? block.add(P.hT) : -1;
        const size_t tableSize = (size_t)P.up * P.taps;
        ExportStage stage(b, st, block, &b->resampleOrder, !in.sig, in.sig != nullptr);
        if (stage.begin([&] {
                if (tableSize <= b->dResample.cap) return 0;
                if (b->resampleOrder.used) { HIP_TRY(hipEventSynchronize(b->resampleOrder.done)); }      // (the table is freed: its readers first)
                return b->dResample.reserve(tableSize);
            })) return -1;
        if (upload) HIP_TRY(hipMemcpyAsync(b->dResample.ptr, stage.device<float>(tableAt), tableSize * sizeof(float), hipMemcpyDeviceToDevice, st));
        ResArgs A;
        A.in = in.data; A.rows = stage.device<ResRow>(rowsAt);
        A.tile = tile_out(stage, wordsAt, tiles, rowStride, deviceOut);
        A.hT = b->dResample.ptr; A.up = P.up; A.down = P.down; A.Z = P.Z; A.span = res_span(P);
        void (*const kernels[2][2])(ResArgs) = {{klatt_resample<false, int16_t>, klatt_resample<true, int16_t>}, {klatt_resample<false, float>, klatt_resample<true, float>}};
        if (launch_tiles(stage, kernels, in.format(), format, 8, A)) return -1;
        b->resOnDevice = true;
        return elements;
    });
}

long long speechPlayer_batch_exportResampled(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int outRate, int zeros,
                                             double rolloff, int window, double beta, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportResampled")) return -1;
    const long long done = resampled_export("exportResampled", batch, false, nullptr, utterances, nUtterances,
                                            0, outRate, zeros, rolloff, window, beta, deviceOut, format, rowStride, stream);
    return done == -2 ? speechPlayer_batch_exportPcm(batch, utterances, nUtterances, deviceOut, format, rowStride, stream) : done;
}

// The same of chosen rows of a caller's signal at `srcRate`: it reads no pool and needs no synthesis (ExportStage, ofSignal); the table is
// the batch's, keyed by the source rate as well, in the shared order.
long long speechPlayer_batch_exportResampledOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int srcRate,
                                               int outRate, int zeros, double rolloff, int window, double beta, void* deviceOut, int format, long long rowStride,
                                               void* stream)
{
    const char* what = "exportResampledOf";
    if (refuse_timing_only("speechPlayer_batch_exportResampledOf")) return -1;
    return resampled_export(what, batch, true, signal, rows, nRows,
                            srcRate, outRate, zeros, rolloff, window, beta, deviceOut, format, rowStride, stream);
}

// ---- the PCM convolved with impulse responses (klatt_convolve.h) -------------------------------------------------------------------------
// Host only, touches no device: the definition of include/speechPlayer_batch.h through the functions the kernel is compiled from.
static long long convolve_statement(const char* what, const void* x, int inFormat, long long length, const float* ir, long long taps, int tail, int format, void* out,
                                    long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || (length > 0 && !x)) { set_error("%s: length %lld (0 .. 2^44, with its samples)", what, length); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    try {
        ConvPlan P;
        std::string why;
        const long long starts[2] = {0, taps};
        if (!conv_plan(P, ir, starts, 1, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        const long long Lout = conv_length(length, taps, tail);
        if (!out) return Lout;
        if (capacity < Lout) { set_error("%s: the output takes %lld elements, capacity is %lld", what, Lout, capacity); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? convolve_host(static_cast<const float*>(x), length, P.taps.data(), taps, tail, format, out)
                        : convolve_host(static_cast<const int16_t*>(x), length, P.taps.data(), taps, tail, format, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmConvolve(const sample* pcm, long long length, const float* ir, long long taps, int tail, int format, void* out,
                                   long long capacity)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return convolve_statement("pcmConvolve", pcm, 0, length, ir, taps, tail, format, out, capacity);
}

long long speechPlayer_signalConvolve(const void* x, int inFormat, long long length, const float* ir, long long taps, int tail, int format, void* out,
                                      long long capacity)
{
    begin_call();
    return convolve_statement("signalConvolve", x, inFormat, length, ir, taps, tail, format, out, capacity);
}

// Tiles cost in proportion to their response's taps: many more workgroups than the device holds at once, so that the dispatcher evens out
// what a fixed share per workgroup would not (the whole-row export and the stage alike).
constexpr long long kConvolveGroupsPerCu = 64;

// The chosen utterances' PCM, each row through the response irOf names (klatt_convolve.h).  It reads the pool, so it is ordered as
// speechPlayer_batch_exportPcm is (ExportStage, ofPcm), tile-wise; the rows carry their response as well.  The staging block: rows | tile
// starts and chunk rows (packed) | the responses.  Nothing is kept on the batch: the kernel reads the responses from the call's own slot.
// ofSignal and `signal` as spectrogram_export's.
static long long convolved_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances, const float* ir,
                                  const long long* irStart, long long nIr, const long long* irOf, int tail, void* deviceOut, int format,
                                  long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        ConvPlan P;
        std::string why;
        if (!conv_plan(P, ir, irStart, nIr, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<ConvRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                const long long j = conv_row(P, irOf, i, why);
                if (j < 0) { set_error("%s: %s", what, why.c_str()); return -1; }
                const long long L = in.len(u), K = P.start[(size_t)j + 1] - P.start[(size_t)j], Lout = conv_length(L, K, tail);
                rows.push_back(ConvRow{in.at(u), L, Lout, tile_row_first(i, rowStride, before), P.start[(size_t)j], K});
                return Lout;
            }, in.sig)) return -1;
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        std::vector<long long> words;
        const TileTable tiles = tile_row_table(s.counts.data(), s.n, kConvolveTile, rowStride, kTimelineChunkLog2, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), tapsAt = block.add(P.taps);
        ExportStage stage(b, static_cast<hipStream_t>(stream), block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        ConvArgs A;
        A.in = in.data; A.rows = stage.device<ConvRow>(rowsAt);
        A.tile = tile_out(stage, wordsAt, tiles, rowStride, deviceOut);
        A.taps = stage.device<float>(tapsAt);
        void (*const kernels[2][2])(ConvArgs) = {{klatt_convolve<false, int16_t>, klatt_convolve<true, int16_t>}, {klatt_convolve<false, float>, klatt_convolve<true, float>}};
        if (launch_tiles(stage, kernels, in.format(), format, kConvolveGroupsPerCu, A)) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportConvolved(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const float* ir,
                                             const long long* irStart, long long nIr, const long long* irOf, int tail, void* deviceOut, int format,
                                             long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportConvolved")) return -1;
    return convolved_export("exportConvolved", batch, false, nullptr, utterances, nUtterances,
                            ir, irStart, nIr, irOf, tail, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal, irOf per output row: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportConvolvedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
                                               const float* ir, const long long* irStart, long long nIr, const long long* irOf, int tail, void* deviceOut,
                                               int format, long long rowStride, void* stream)
{
    const char* what = "exportConvolvedOf";
    if (refuse_timing_only("speechPlayer_batch_exportConvolvedOf")) return -1;
    return convolved_export(what, batch, true, signal, rows, nRows,
                            ir, irStart, nIr, irOf, tail, deviceOut, format, rowStride, stream);
}

// ---- the PCM through cascades of biquad sections (klatt_filter.h) ---------------------------------------------------------------------------
static_assert(sizeof(FilterRow) % 8 == 0 && sizeof(FilterGroup) % 8 == 0 && sizeof(FilterSection) == 20, "rows and groups are arrays of 8-byte words, a section is five floats");

// Host only, touches no device: the definition of include/speechPlayer_batch.h through the functions the kernel is compiled from.
static long long filter_statement(const char* what, const void* x, int inFormat, long long length, const float* sections, long long nSections, long long tail, int format,
                                  void* out, long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || (length > 0 && !x)) { set_error("%s: length %lld (0 .. 2^44, with its samples)", what, length); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    try {
        FilterPlan P;
        std::string why;
        const long long starts[2] = {0, nSections};
        if (!filter_plan(P, sections, starts, 1, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        const long long Lout = filter_length(length, tail);
        if (!out) return Lout;
        if (capacity < Lout) { set_error("%s: the output takes %lld elements, capacity is %lld", what, Lout, capacity); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? filter_host(static_cast<const float*>(x), length, P.sections.data(), nSections, tail, format, out)
                        : filter_host(static_cast<const int16_t*>(x), length, P.sections.data(), nSections, tail, format, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmFilter(const sample* pcm, long long length, const float* sections, long long nSections, long long tail, int format, void* out,
                                 long long capacity)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return filter_statement("pcmFilter", pcm, 0, length, sections, nSections, tail, format, out, capacity);
}

long long speechPlayer_signalFilter(const void* x, int inFormat, long long length, const float* sections, long long nSections, long long tail, int format,
                                    void* out, long long capacity)
{
    begin_call();
    return filter_statement("signalFilter", x, inFormat, length, sections, nSections, tail, format, out, capacity);
}

// The entry point on filter_rows that takes these arguments: the whole-row export's, or the stage's that keeps state (klatt_stage.h)
extern "C++" template <int K, bool F32, typename In> static void (*filter_entry(const FilterArgs&))(FilterArgs) { return klatt_filter<K, F32, In>; }
extern "C++" template <int K, bool F32, typename In> static void (*filter_entry(const StageFilterArgs&))(StageFilterArgs) { return klatt_stage_filter<K, F32, In>; }

// ... its instantiation for a bucket, an input format and an output format
extern "C++" template <int K, class Args>
static void (*filter_kernel(int inFormat, int format, const Args& A))(Args)
{
    void (*const kernels[2][2])(Args) = {{filter_entry<K, false, int16_t>(A), filter_entry<K, true, int16_t>(A)}, {filter_entry<K, false, float>(A), filter_entry<K, true, float>(A)}};
    return kernels[inFormat][format];
}

// The launches of a packed table's groups on the stage's stream, one per bucket that has groups (those of one bucket lie together); A holds
// everything but the groups, which are the block's section groupsAt.  A wavefront per group; no more workgroups than keep every SIMD of the
// device busy several times over.
extern "C++" template <class Args>
static int launch_filter_groups(const ExportStage& stage, const std::vector<FilterGroup>& groups, int groupsAt, int inFormat, int format, Args& A)
{
    for (size_t first = 0; first < groups.size();) {
        size_t end = first;
        while (end < groups.size() && groups[end].bucket == groups[first].bucket) ++end;
        A.groups = stage.device<FilterGroup>(groupsAt) + first;
        A.nGroups = (long long)(end - first);
        void (*kernel)(Args) = nullptr;
        switch (groups[first].bucket) {
            case 1: kernel = filter_kernel<1>(inFormat, format, A); break;
            case 2: kernel = filter_kernel<2>(inFormat, format, A); break;
            case 4: kernel = filter_kernel<4>(inFormat, format, A); break;
            case 8: kernel = filter_kernel<8>(inFormat, format, A); break;
            default: kernel = filter_kernel<16>(inFormat, format, A); break;
        }
        const unsigned grid = (unsigned)std::min<long long>(A.nGroups, 64ll * stage.b->cus);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kFilterLanes), 0, stage.st, A);
        HIP_TRY(hipGetLastError());
        first = end;
    }
    return 0;
}

// The chosen utterances' PCM, each row through the filter filterOf names (klatt_filter.h).  It reads the pool, so it is ordered as
// speechPlayer_batch_exportPcm is (ExportStage, ofPcm).  A wavefront takes 64 rows, not tiles of one: the rows are packed into groups
// (filter_pack) and carry their first element in the output, so there is no tile table; one launch per bucket that has groups.  The
// staging block: packed rows | groups | the sections.  Nothing is kept on the batch.  ofSignal and `signal` as spectrogram_export's.
static long long filtered_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances,
                                 const float* sections, const long long* secStart, long long nFilters, const long long* filterOf, long long tail, void* deviceOut,
                                 int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        FilterPlan P;
        std::string why;
        if (!filter_plan(P, sections, secStart, nFilters, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<FilterRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                const long long j = filter_row(P, filterOf, i, why);
                if (j < 0) { set_error("%s: %s", what, why.c_str()); return -1; }
                const long long L = in.len(u), Lout = filter_length(L, tail);
                rows.push_back(FilterRow{in.at(u), L, Lout, tile_row_first(i, rowStride, before), P.start[(size_t)j], P.start[(size_t)j + 1] - P.start[(size_t)j]});
                return Lout;
            }, in.sig)) return -1;
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        std::vector<FilterRow> packed;
        std::vector<FilterGroup> groups;
        filter_pack(rows, packed, groups);
        StageBlock block;
        const int rowsAt = block.add(packed), groupsAt = block.add(groups), sectionsAt = block.add(P.sections);
        ExportStage stage(b, static_cast<hipStream_t>(stream), block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        FilterArgs A;
        A.in = in.data; A.rows = stage.device<FilterRow>(rowsAt);
        A.sections = stage.device<FilterSection>(sectionsAt);
        A.rowStride = rowStride; A.out = deviceOut;
        if (launch_filter_groups(stage, groups, groupsAt, in.format(), format, A) || stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportFiltered(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const float* sections,
                                            const long long* secStart, long long nFilters, const long long* filterOf, long long tail, void* deviceOut, int format,
                                            long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportFiltered")) return -1;
    return filtered_export("exportFiltered", batch, false, nullptr, utterances, nUtterances,
                           sections, secStart, nFilters, filterOf, tail, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal, filterOf per output row: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportFilteredOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
                                              const float* sections, const long long* secStart, long long nFilters, const long long* filterOf, long long tail,
                                              void* deviceOut, int format, long long rowStride, void* stream)
{
    const char* what = "exportFilteredOf";
    if (refuse_timing_only("speechPlayer_batch_exportFilteredOf")) return -1;
    return filtered_export(what, batch, true, signal, rows, nRows,
                           sections, secStart, nFilters, filterOf, tail, deviceOut, format, rowStride, stream);
}

// ---- the PCM through the G.711 laws and IMA ADPCM (klatt_codec.h) ---------------------------------------------------------------------------
// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernels are compiled from.
static int codec_request(const char* what, int codec, int format)
{
    if (codec < 0 || codec >= kCodecCount) { set_error("%s: codec %d (0 ulaw, 1 alaw, 2 adpcm)", what, codec); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    return 0;
}

static long long code_statement(const char* what, const void* x, int inFormat, long long length, int codec, int format, void* decodedOut, unsigned char* codesOut,
                                long long capacity, int* state)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || (length > 0 && !x)) { set_error("%s: length %lld (0 .. 2^44, with its samples)", what, length); return -1; }
    if (codec_request(what, codec, format)) return -1;
    if (length > 0 && !decodedOut && !codesOut) { set_error("%s: no output (the decoded samples, the codes or both)", what); return -1; }
    if (capacity < length) { set_error("%s: the output takes %lld elements, capacity is %lld", what, length, capacity); return -1; }
    if (signal_host_values(what, x, inFormat, length)) return -1;
    if (inFormat) code_host(static_cast<const float*>(x), length, codec, format, decodedOut, codesOut, state);
    else code_host(static_cast<const int16_t*>(x), length, codec, format, decodedOut, codesOut, state);
    return length;
}

long long speechPlayer_pcmCode(const sample* pcm, long long length, int codec, int format, void* decodedOut, unsigned char* codesOut, long long capacity, int* state)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return code_statement("pcmCode", pcm, 0, length, codec, format, decodedOut, codesOut, capacity, state);
}

long long speechPlayer_signalCode(const void* x, int inFormat, long long length, int codec, int format, void* decodedOut, unsigned char* codesOut, long long capacity,
                                  int* state)
{
    begin_call();
    return code_statement("signalCode", x, inFormat, length, codec, format, decodedOut, codesOut, capacity, state);
}

long long speechPlayer_codecDecode(const unsigned char* codes, long long length, int codec, int format, void* out, long long capacity, int* state)
{
    begin_call();
    const char* what = "codecDecode";
    if (length < 0 || length > kResampleMaxLength || (length > 0 && !codes)) { set_error("%s: length %lld (0 .. 2^44, with its codes)", what, length); return -1; }
    if (codec_request(what, codec, format)) return -1;
    if (length > 0 && !out) { set_error("%s: no output", what); return -1; }
    if (capacity < length) { set_error("%s: the output takes %lld elements, capacity is %lld", what, length, capacity); return -1; }
    const long long bad = decode_bad_code(codes, length, codec);
    if (bad >= 0) { set_error("%s: code %lld is %d (an ADPCM code is 0 .. 15)", what, bad, (int)codes[bad]); return -1; }
    decode_host(codes, length, codec, format, out, state);
    return length;
}

// klatt_code_g711 of a law (input format, output format) over the tiles, on the stage's stream, at most 8 workgroups per CU
static int launch_g711(const ExportStage& stage, int codec, int inFormat, int format, const CodeArgs& A)
{
    void (*const ulaw[2][2])(CodeArgs) = {{klatt_code_g711<kCodecUlaw, false, int16_t>, klatt_code_g711<kCodecUlaw, true, int16_t>},
                                          {klatt_code_g711<kCodecUlaw, false, float>, klatt_code_g711<kCodecUlaw, true, float>}};
    void (*const alaw[2][2])(CodeArgs) = {{klatt_code_g711<kCodecAlaw, false, int16_t>, klatt_code_g711<kCodecAlaw, true, int16_t>},
                                          {klatt_code_g711<kCodecAlaw, false, float>, klatt_code_g711<kCodecAlaw, true, float>}};
    const unsigned grid = (unsigned)std::min<long long>(A.tile.nTiles, 8ll * stage.b->cus);
    hipLaunchKernelGGL((codec == kCodecUlaw ? ulaw : alaw)[inFormat][format], dim3(grid), dim3(256), 0, stage.st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The entry point on adpcm_rows that takes these arguments: the whole-row export's, or the stage's that keeps state (klatt_stage.h)
extern "C++" template <int OUT, bool F32, typename In> static void (*adpcm_entry(const AdpcmArgs&))(AdpcmArgs) { return klatt_code_adpcm<OUT, F32, In>; }
extern "C++" template <int OUT, bool F32, typename In> static void (*adpcm_entry(const StageAdpcmArgs&))(StageAdpcmArgs) { return klatt_stage_adpcm<OUT, F32, In>; }

// ... its instantiation for (input format, outputs, output format) over A's groups, on the stage's stream: a wavefront per group; no more
// workgroups than keep every SIMD of the device busy several times over
extern "C++" template <class Args>
static int launch_adpcm(const ExportStage& stage, int inFormat, int outputs, int format, const Args& A)
{
    // [input format][outputs - 1][output format]; the codes alone have no output format
    constexpr int D = kCodeDecoded, C = kCodeCodes;
    void (*const kernels[2][3][2])(Args) = {
        {{adpcm_entry<D, false, int16_t>(A), adpcm_entry<D, true, int16_t>(A)}, {adpcm_entry<C, false, int16_t>(A), adpcm_entry<C, false, int16_t>(A)},
         {adpcm_entry<D | C, false, int16_t>(A), adpcm_entry<D | C, true, int16_t>(A)}},
        {{adpcm_entry<D, false, float>(A), adpcm_entry<D, true, float>(A)}, {adpcm_entry<C, false, float>(A), adpcm_entry<C, false, float>(A)},
         {adpcm_entry<D | C, false, float>(A), adpcm_entry<D | C, true, float>(A)}}};
    const unsigned grid = (unsigned)std::min<long long>(A.nGroups, 64ll * stage.b->cus);
    hipLaunchKernelGGL(kernels[inFormat][outputs - 1][format], dim3(grid), dim3(kFilterLanes), 0, stage.st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The chosen utterances' PCM coded (klatt_codec.h): the decoded samples, the codes or both, on one grid.  It reads the pool, so it is ordered
// as speechPlayer_batch_exportPcm is (ExportStage, ofPcm).  A G.711 law goes tile-wise (the staging block: rows | tile starts and chunk rows,
// packed); ADPCM a wavefront per 64 rows as filtered_export's (packed rows | groups).  Nothing is kept on the batch.  ofSignal and `signal` as
// spectrogram_export's.
static long long coded_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances,
                              int codec, void* decodedOut, int format, void* codesOut, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (codec < 0 || codec >= kCodecCount) { set_error("%s: codec %d (0 ulaw, 1 alaw, 2 adpcm)", what, codec); return -1; }
        if (!decodedOut && !codesOut) { set_error("%s: no output (the decoded samples, the codes or both)", what); return -1; }
        if (tile_request(what, format, rowStride)) return -1;
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<FilterRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                const long long L = in.len(u);
                rows.push_back(FilterRow{in.at(u), L, L, tile_row_first(i, rowStride, before), 0, 1});
                return L;
            }, in.sig)) return -1;
        const long long elements = export_elements(what, kSampleNouns, s, rowStride, 1);
        if (elements <= 0) return elements;
        if (!in.sig && export_synthesised(b, what)) return -1;
        const size_t elSize = format ? sizeof(float) : sizeof(int16_t);
        if (decodedOut && (export_output(b, what, decodedOut, elements, elSize) || signal_memory(in, what, decodedOut, (size_t)elements * elSize))) return -1;
        if (codesOut && (export_output(b, what, codesOut, elements, 1) || signal_memory(in, what, codesOut, (size_t)elements))) return -1;
        if (decodedOut && codesOut) {
            const uintptr_t d = reinterpret_cast<uintptr_t>(decodedOut), c = reinterpret_cast<uintptr_t>(codesOut);
            if (d < c + (size_t)elements && c < d + (size_t)elements * elSize) { set_error("%s: the decoded samples and the codes overlap", what); return -1; }
        }
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (codec != kCodecAdpcm) {
            std::vector<ResRow> tileRows;
            tileRows.reserve(rows.size());
            for (const FilterRow& r : rows) tileRows.push_back(ResRow{r.src, r.len, r.outLen, r.dst});
            std::vector<long long> words;
            const TileTable tiles = tile_row_table(s.counts.data(), s.n, kCodeTile, rowStride, kTimelineChunkLog2, words);
            StageBlock block;
            const int rowsAt = block.add(tileRows), wordsAt = block.add(words);
            ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
            if (stage.begin()) return -1;
            CodeArgs A;
            A.in = in.data; A.rows = stage.device<ResRow>(rowsAt);
            A.tile = tile_out(stage, wordsAt, tiles, rowStride, decodedOut);
            A.codes = static_cast<uint8_t*>(codesOut);
            if (launch_g711(stage, codec, in.format(), format, A) || stage.finish()) return -1;
            return elements;
        }
        std::vector<FilterRow> packed;
        std::vector<FilterGroup> groups;
        filter_pack(rows, packed, groups);
        StageBlock block;
        const int rowsAt = block.add(packed), groupsAt = block.add(groups);
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        AdpcmArgs A;
        A.in = in.data; A.rows = stage.device<FilterRow>(rowsAt);
        A.groups = stage.device<FilterGroup>(groupsAt); A.nGroups = (long long)groups.size();
        A.rowStride = rowStride; A.decoded = decodedOut; A.codes = static_cast<uint8_t*>(codesOut);
        const int outputs = (decodedOut ? kCodeDecoded : 0) | (codesOut ? kCodeCodes : 0);
        if (launch_adpcm(stage, in.format(), outputs, format, A) || stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportCoded(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int codec, void* decodedOut, int format,
                                         unsigned char* codesOut, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportCoded")) return -1;
    return coded_export("exportCoded", batch, false, nullptr, utterances, nUtterances, codec, decodedOut, format, codesOut, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportCodedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int codec,
                                           void* decodedOut, int format, unsigned char* codesOut, long long rowStride, void* stream)
{
    const char* what = "exportCodedOf";
    if (refuse_timing_only("speechPlayer_batch_exportCodedOf")) return -1;
    return coded_export(what, batch, true, signal, rows, nRows, codec, decodedOut, format, codesOut, rowStride, stream);
}

// ---- signal stages (klatt_stage.h, klatt_stage_window.h): the resampler, the filter, the codecs, the convolution and the spectrogram chunk by chunk ----
static_assert(sizeof(StageHistRow) % 8 == 0 && sizeof(StageResRow) % 8 == 0 && sizeof(StageLaneRow) % 8 == 0, "rows are arrays of 8-byte words");

// Host only, touches no device: the outputs a resampler stage has emitted after `consumed` samples of a row, open or ended
long long speechPlayer_resampleEmitted(long long consumed, int srcRate, int outRate, int zeros, double rolloff, int ended)
{
    begin_call();
    const char* what = "resampleEmitted";
    if (consumed < 0 || consumed > kResampleMaxLength) { set_error("%s: %lld samples consumed (0 .. 2^44)", what, consumed); return -1; }
    try {
        ResPlan P;
        std::string why;
        if (!res_plan(P, srcRate, outRate, zeros, rolloff, 0, 0.0, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        return stage_res_emitted(consumed, P.identity ? 0 : P.Z, P.up, P.down, ended != 0);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

// A stage of nRows rows on `batch`: fill(b, s) plans it and makes its state (+0) on the device; then it is the batch's and a live handle
extern "C++" template <class Fill>
static speechPlayer_stage_t stage_create(const char* what, speechPlayer_batch_t batch, long long nRows, Fill fill)
{
    begin_call();
    Batch* b = static_cast<Batch*>(batch);
    if (!b) { set_error("%s: no batch", what); return nullptr; }
    if (nRows < 1 || nRows > kStageMaxRows) { set_error("%s: nRows %lld (1 .. 2^20)", what, nRows); return nullptr; }
    Stage* s = nullptr;
    try {
        s = new Stage;
        s->nRows = nRows;
        s->N.assign((size_t)nRows, 0); s->M.assign((size_t)nRows, 0); s->histAt.assign((size_t)nRows + 1, 0);
        const auto made = [&]() -> int {
            if (fill(b, s)) return -1;
            HIP_TRY(hipSetDevice(b->device));
            HIP_TRY(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
            HIP_TRY(hipStreamSynchronize(b->stream));      // (the state's zeros are there)
            return 0;
        };
        if (made()) { stage_release(s); return nullptr; }
        s->b = b;
        b->stages.push_back(s);
        std::lock_guard<std::mutex> lock(g_stageMutex);
        g_stages.push_back(s);
        return s;
    } catch (const std::exception& e) {
        set_error("%s: %s", what, e.what());
        if (s) stage_release(s);
        return nullptr;
    }
}
// n dwords of +0 on the batch's device, behind the batch's stream
extern "C++" template <class T>
static int stage_zeros(Batch* b, DeviceBuffer<T>& buf, size_t n)
{
    static_assert(sizeof(T) == 4, "a state is dwords");
    HIP_TRY(hipSetDevice(b->device));
    if (buf.reserve(n)) return -1;
    HIP_TRY(hipMemsetAsync(buf.ptr, 0, n * sizeof(T), b->stream));
    return 0;
}
// The histories of a stage whose kind keeps one, row r's H(r) float32 from histAt[r] of either buffer: refused beyond `cap` samples in all
// (kStageMaxHistory, the convolution's and the spectrogram's) before anything is allocated
constexpr long long kStageNoCap = 0x7FFFFFFFFFFFFFFFll;      // the resampler's cap: its histories are 2^20 rows of 1023 samples at the most and are not refused
extern "C++" template <class Len>
static int stage_histories(const char* what, Batch* b, Stage* s, Len H, long long cap)
{
    for (long long i = 0; i < s->nRows; ++i) {
        const long long h = H(i);
        if (h > cap - s->histAt[(size_t)i]) {
            int bits = 0;      // (a cap is a power of two)
            while ((1ll << bits) < cap) ++bits;
            set_error("%s: the rows' histories take more than 2^%d samples in all (row %lld keeps %lld)", what, bits, i, h);
            return -1;
        }
        s->histAt[(size_t)i + 1] = s->histAt[(size_t)i] + h;
        s->mostHistory = std::max(s->mostHistory, h);
    }
    const size_t n = (size_t)s->histAt[(size_t)s->nRows];
    return n == 0 ? 0 : stage_zeros(b, s->dHist[0], n) || stage_zeros(b, s->dHist[1], n) ? -1 : 0;
}

speechPlayer_stage_t speechPlayer_batch_stageResample(speechPlayer_batch_t batch, long long nRows, int srcRate, int outRate, int zeros, double rolloff, int window, double beta)
{
    const char* what = "stageResample";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        std::string why;
        if (!res_plan(s->res, srcRate, outRate, zeros, rolloff, window, beta, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        ResPlan& P = s->res;
        s->g.kind = kStageResample; s->g.up = P.up; s->g.down = P.down; s->g.Z = P.identity ? 0 : P.Z;
        const long long H = stage_history(s->g.Z);
        if (stage_histories(what, b, s, [&](long long) { return H; }, kStageNoCap)) return -1;
        if (P.identity) return 0;      // equal rates: no table, and histories of no samples
        res_transpose(P);
        HIP_TRY(hipSetDevice(b->device));
        if (s->dTable.reserve(P.hT.size())) return -1;
        HIP_TRY(hipMemcpy(s->dTable.ptr, P.hT.data(), P.hT.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<float>().swap(P.table); std::vector<float>().swap(P.hT);      // (the device holds what the pushes read)
        return 0;
    });
}

speechPlayer_stage_t speechPlayer_batch_stageFilter(speechPlayer_batch_t batch, long long nRows, const float* sections, const long long* secStart, long long nFilters,
                                                    const long long* filterOf, long long tail)
{
    const char* what = "stageFilter";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        std::string why;
        if (!filter_plan(s->fil, sections, secStart, nFilters, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        s->g.kind = kStageFilter; s->g.tail = tail;
        s->secAt.resize((size_t)s->nRows); s->secN.resize((size_t)s->nRows);
        for (long long i = 0; i < s->nRows; ++i) {
            const long long j = filter_row(s->fil, filterOf, i, why);
            if (j < 0) { set_error("%s: %s", what, why.c_str()); return -1; }
            s->secAt[(size_t)i] = s->fil.start[(size_t)j];
            s->secN[(size_t)i] = s->fil.start[(size_t)j + 1] - s->fil.start[(size_t)j];
        }
        return stage_zeros(b, s->dFilterState, (size_t)s->nRows * kStageFilterState);
    });
}

speechPlayer_stage_t speechPlayer_batch_stageCode(speechPlayer_batch_t batch, long long nRows, int codec)
{
    const char* what = "stageCode";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        if (codec < 0 || codec >= kCodecCount) { set_error("%s: codec %d (0 ulaw, 1 alaw, 2 adpcm)", what, codec); return -1; }
        s->g.kind = kStageCode; s->codec = codec;
        return codec == kCodecAdpcm ? stage_zeros(b, s->dCodeState, (size_t)s->nRows * 2) : 0;      // (the G.711 laws carry no state)
    });
}

extern "C++" template <class T>
static int stage_upload(Batch* b, DeviceBuffer<T>& buf, const std::vector<T>& v)
{
    if (v.empty()) return 0;
    HIP_TRY(hipSetDevice(b->device));
    if (buf.reserve(v.size())) return -1;
    HIP_TRY(hipMemcpy(buf.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

speechPlayer_stage_t speechPlayer_batch_stageConvolve(speechPlayer_batch_t batch, long long nRows, const float* ir, const long long* irStart, long long nIr,
                                                      const long long* irOf, int tail)
{
    const char* what = "stageConvolve";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        ConvPlan P;
        std::string why;
        if (!conv_plan(P, ir, irStart, nIr, tail, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        s->g.kind = kStageConvolve; s->g.tail = tail;
        s->irAt.resize((size_t)s->nRows);
        std::vector<long long> taps((size_t)s->nRows);
        for (long long i = 0; i < s->nRows; ++i) {
            const long long j = conv_row(P, irOf, i, why);
            if (j < 0) { set_error("%s: %s", what, why.c_str()); return -1; }
            s->irAt[(size_t)i] = P.start[(size_t)j];
            taps[(size_t)i] = P.start[(size_t)j + 1] - P.start[(size_t)j];
        }
        if (stage_histories(what, b, s, [&](long long i) { return (long long)stage_conv_history(taps[(size_t)i]); }, kStageMaxHistory)) return -1;
        return stage_upload(b, s->dTaps, P.taps);
    });
}

// hop and phase of a stage's step grid: a row may consume 2^44 samples, so a larger hop or phase means the same as kStageMaxStep = 2^45
// (the whole-row exports, whose rows are shorter, stop at 2^40)
static int stage_step_request(const char* what, long long& hop, long long& phase)
{
    if (hop <= 0 || phase < 0) { set_error("%s: hop %lld, phase %lld", what, hop, phase); return -1; }
    hop = std::min(hop, kStageMaxStep); phase = std::min(phase, kStageMaxStep);
    return 0;
}

speechPlayer_stage_t speechPlayer_batch_stageSpectrogram(speechPlayer_batch_t batch, long long nRows, int nFft, long long hop, long long phase, const double* window,
                                                         const double* bank, int nBands, int power, double logScale, double floor)
{
    const char* what = "stageSpectrogram";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        if (stage_step_request(what, hop, phase)) return -1;
        SpecPlan& P = s->spec;
        std::string why;
        if (!spec_plan(P, nFft, window, bank, nBands, power, logScale, floor, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        s->g.kind = kStageSpectrogram; s->g.frames = stage_spec_frames(nFft, hop, phase);
        const long long H = stage_frame_history(s->g.frames);
        if (stage_histories(what, b, s, [&](long long) { return H; }, kStageMaxHistory)) return -1;
        if (stage_upload(b, s->dWindow, P.window) || stage_upload(b, s->dTw, P.tw) || stage_upload(b, s->dWeights, P.weights) || stage_upload(b, s->dRange, P.range)) return -1;
        std::vector<float>().swap(P.window); std::vector<SpecCx>().swap(P.tw); std::vector<float>().swap(P.weights); std::vector<int>().swap(P.range);      // (the device holds what the pushes read)
        return 0;
    });
}

// Host only, touches no device: the steps a spectrogram stage has emitted after `consumed` samples of a row, open or ended
long long speechPlayer_spectrogramEmitted(long long consumed, int nFft, long long hop, long long phase, int ended)
{
    begin_call();
    const char* what = "spectrogramEmitted";
    if (consumed < 0 || consumed > kResampleMaxLength) { set_error("%s: %lld samples consumed (0 .. 2^44)", what, consumed); return -1; }
    if (nFft < kSpecMinFft || nFft > kSpecMaxFft || (nFft & (nFft - 1))) { set_error("%s: nFft %d (a power of two in %d .. %d)", what, nFft, kSpecMinFft, kSpecMaxFft); return -1; }
    if (stage_step_request(what, hop, phase)) return -1;
    return stage_frames_emitted(stage_spec_frames(nFft, hop, phase), consumed, ended != 0);
}

// The stages on the step grid (klatt_stage_frames.h): the whole-row exports' plans, a history of the frame's before + after samples a row
speechPlayer_stage_t speechPlayer_batch_stageLpc(speechPlayer_batch_t batch, long long nRows, int order, int nWin, long long hop, long long phase, const double* window,
                                                 const double* lagWindow, int fields)
{
    const char* what = "stageLpc";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        if (stage_step_request(what, hop, phase)) return -1;
        LpcPlan& P = s->lpc;
        std::string why;
        if (!lpc_plan(P, order, nWin, window, lagWindow, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        s->g.kind = kStageLpc; s->g.frames = stage_lpc_frames(nWin, hop, phase);
        const long long H = stage_frame_history(s->g.frames);
        if (stage_histories(what, b, s, [&](long long) { return H; }, kStageMaxHistory)) return -1;
        if (stage_upload(b, s->dWindow, P.window) || stage_upload(b, s->dLag, P.lag)) return -1;
        std::vector<float>().swap(P.window); std::vector<double>().swap(P.lag);      // (the device holds what the pushes read)
        return 0;
    });
}

speechPlayer_stage_t speechPlayer_batch_stagePitch(speechPlayer_batch_t batch, long long nRows, int sampleRate, int nWin, int lagMin, int lagMax, double threshold,
                                                   long long hop, long long phase, int fields)
{
    const char* what = "stagePitch";
    return stage_create(what, batch, nRows, [&](Batch* b, Stage* s) -> int {
        if (stage_step_request(what, hop, phase)) return -1;
        std::string why;
        if (!pitch_plan(s->pitch, sampleRate, nWin, lagMin, lagMax, threshold, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        s->g.kind = kStagePitch; s->g.frames = stage_pitch_frames(nWin, lagMax, hop, phase);
        const long long H = stage_frame_history(s->g.frames);
        return stage_histories(what, b, s, [&](long long) { return H; }, kStageMaxHistory);
    });
}

// Host only, touch no device: the steps an LPC or a pitch stage has emitted after `consumed` samples of a row, open or ended
static long long stage_emitted_request(const char* what, long long consumed, long long& hop, long long& phase)
{
    if (consumed < 0 || consumed > kResampleMaxLength) { set_error("%s: %lld samples consumed (0 .. 2^44)", what, consumed); return -1; }
    return stage_step_request(what, hop, phase);
}

long long speechPlayer_lpcEmitted(long long consumed, int nWin, long long hop, long long phase, int ended)
{
    begin_call();
    const char* what = "lpcEmitted";
    if (stage_emitted_request(what, consumed, hop, phase)) return -1;
    if (nWin < 2 || nWin > kLpcMaxWin) { set_error("%s: nWin %d (2 .. %d)", what, nWin, kLpcMaxWin); return -1; }
    return stage_frames_emitted(stage_lpc_frames(nWin, hop, phase), consumed, ended != 0);
}

long long speechPlayer_pitchEmitted(long long consumed, int nWin, int lagMax, long long hop, long long phase, int ended)
{
    begin_call();
    const char* what = "pitchEmitted";
    if (stage_emitted_request(what, consumed, hop, phase)) return -1;
    if (nWin < kPitchMinWin || nWin > kPitchMaxWin) { set_error("%s: nWin %d (%d .. %d)", what, nWin, kPitchMinWin, kPitchMaxWin); return -1; }
    if (lagMax < 3 || lagMax > kPitchMaxLag) { set_error("%s: lagMax %d (3 .. %d)", what, lagMax, kPitchMaxLag); return -1; }
    return stage_frames_emitted(stage_pitch_frames(nWin, lagMax, hop, phase), consumed, ended != 0);
}

// The stage a handle names, or null with the message set: a handle that was freed -- alone or with its batch -- names none
static Stage* stage_of(const char* what, speechPlayer_stage_t stage)
{
    Stage* s = static_cast<Stage*>(stage);
    if (!s) { set_error("%s: no stage", what); return nullptr; }
    if (!stage_known(s)) { set_error("%s: %p is not a stage (freed, alone or with its batch?)", what, stage); return nullptr; }
    return s;
}

// What a push of rows of len(i) samples with these end flags emits per row (stage_row_plan), as an export's selection; -1 with the message set
extern "C++" template <class Len>
static int stage_selection(const char* what, const Stage* s, Len len, const unsigned char* end, ExportSelection& sel)
{
    sel.n = s->nRows;
    sel.counts.resize((size_t)s->nRows);
    for (long long i = 0; i < s->nRows; ++i) {
        const long long c = len(i);
        long long out;
        if (!stage_row_plan(s->g, s->histAt[(size_t)i + 1] - s->histAt[(size_t)i], s->N[(size_t)i], s->M[(size_t)i], c, end && end[i], out)) {
            set_error("%s: row %lld has consumed %lld samples and would take %lld more (0 or more, at most 2^44 in all)", what, i, s->N[(size_t)i], c);
            return -1;
        }
        sel.counts[(size_t)i] = out;
        sel.most = std::max(sel.most, out);
        sel.total += out;
    }
    return 0;
}

long long speechPlayer_stage_plan(speechPlayer_stage_t stage, const long long* lengths, const unsigned char* end, long long* outLengths)
{
    begin_call();
    const char* what = "stage_plan";
    Stage* s = stage_of(what, stage);
    if (!s) return -1;
    if (!lengths) { set_error("%s: no lengths", what); return -1; }
    try {
        ExportSelection sel;
        if (stage_selection(what, s, [&](long long i) { return lengths[i]; }, end, sel)) return -1;
        for (long long i = 0; outLengths && i < s->nRows; ++i) outLengths[i] = sel.counts[(size_t)i];
        return sel.total;
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

// One push's passage through a slot: ExportStage over a signal, behind the stage's last push whichever stream that was on
extern "C++" struct StagePass {
    Stage* s;
    ExportStage stage;
    StagePass(Stage* s, hipStream_t st, const StageBlock& block) : s(s), stage(s->b, st, block, nullptr, false, true) {}
    template <class Grow>
    int begin(Grow grow)
    {
        if (stage.begin(grow)) return -1;
        if (s->used) HIP_TRY(hipStreamWaitEvent(stage.st, s->done, 0));
        return 0;
    }
    int begin() { return begin([] { return 0; }); }
    int finish()
    {
        HIP_TRY(hipEventRecord(s->done, stage.st));
        s->used = true;
        return stage.finish();
    }
};

// The rows of a filter or ADPCM stage's push, packed into wavefronts (filter_pack)
static void stage_lane_rows(const Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, long long rowStride,
                            std::vector<StageLaneRow>& packed, std::vector<FilterGroup>& groups)
{
    std::vector<StageLaneRow> rows((size_t)s->nRows);
    long long before = 0;
    for (long long i = 0; i < s->nRows; ++i) {
        StageLaneRow& r = rows[(size_t)i];
        r.src = in.at(i); r.len = in.len(i); r.outLen = sel.counts[(size_t)i]; r.dst = tile_row_first(i, rowStride, before);
        r.secAt = s->g.kind == kStageFilter ? s->secAt[(size_t)i] : 0;
        r.sections = s->g.kind == kStageFilter ? s->secN[(size_t)i] : 1;
        r.state = i; r.ended = end && end[i];
        before += r.outLen;
    }
    filter_pack(rows, packed, groups);
}
// The rows of a push that carries no state, for the whole-row kernels: the resampler's at equal rates, the G.711 laws'
static std::vector<ResRow> stage_plain_rows(const Stage* s, const ExportInput& in, const ExportSelection& sel, long long rowStride)
{
    std::vector<ResRow> rows((size_t)s->nRows);
    long long before = 0;
    for (long long i = 0; i < s->nRows; ++i) {
        rows[(size_t)i] = ResRow{in.at(i), in.len(i), sel.counts[(size_t)i], tile_row_first(i, rowStride, before)};
        before += sel.counts[(size_t)i];
    }
    return rows;
}
// The rows of a push onto a stage whose rows carry their history's place (the convolution, the spectrogram)
static std::vector<StageHistRow> stage_history_rows(const Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, long long rowStride)
{
    std::vector<StageHistRow> rows((size_t)s->nRows);
    long long before = 0;
    for (long long i = 0; i < s->nRows; ++i) {
        rows[(size_t)i] = StageHistRow{in.at(i), in.len(i), s->N[(size_t)i], s->M[(size_t)i], sel.counts[(size_t)i], tile_row_first(i, rowStride, before), end && end[i],
                                       s->histAt[(size_t)i], s->histAt[(size_t)i + 1] - s->histAt[(size_t)i], s->g.kind == kStageConvolve ? s->irAt[(size_t)i] : 0};
        before += sel.counts[(size_t)i];
    }
    return rows;
}
// The next history of every row, into the buffer nothing of this push reads, behind the push's kernel; then the buffers change places
static int stage_history_finish(Stage* s, StagePass& pass, const ExportInput& in, const StageHistRow* dRows)
{
    if (s->mostHistory > 0) {
        const dim3 hgrid((unsigned)std::min<long long>((s->mostHistory + 255) / 256, 64), (unsigned)std::min<long long>(s->nRows, 16ll * s->b->cus));
        hipLaunchKernelGGL(in.format() ? klatt_stage_history_rows<float> : klatt_stage_history_rows<int16_t>, hgrid, dim3(256), 0, pass.stage.st, in.data, dRows, s->nRows,
                           s->dHist[s->cur].ptr, s->dHist[s->cur ^ 1].ptr);
        HIP_TRY(hipGetLastError());
    }
    if (pass.finish()) return -1;
    if (s->mostHistory > 0) s->cur ^= 1;
    return 0;
}

static int stage_push_resample(Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, long long elements, void* deviceOut, int format,
                               long long rowStride, hipStream_t st)
{
    std::vector<long long> words;
    const TileTable tiles = tile_row_table(sel.counts.data(), sel.n, kResampleTile, rowStride, kTimelineChunkLog2, words);
    StageBlock block;
    if (s->g.Z == 0) {      // equal rates: no state, the copy kernel of the whole-row export
        if (elements == 0) return 0;
        const std::vector<ResRow> rows = stage_plain_rows(s, in, sel, rowStride);
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        StagePass pass(s, st, block);
        if (pass.begin()) return -1;
        return launch_signal_copy(pass.stage, in, format, pass.stage.device<ResRow>(rowsAt), tile_out(pass.stage, wordsAt, tiles, rowStride, deviceOut)) || pass.finish() ? -1 : 0;
    }
    // The resampler's own 56-byte rows (klatt_stage.h, StageResRow): its histories' places follow from the row's number
    std::vector<StageResRow> rows((size_t)s->nRows);
    long long before = 0;
    for (long long i = 0; i < s->nRows; ++i) {
        rows[(size_t)i] = StageResRow{in.at(i), in.len(i), s->N[(size_t)i], s->M[(size_t)i], sel.counts[(size_t)i], tile_row_first(i, rowStride, before), end && end[i]};
        before += sel.counts[(size_t)i];
    }
    const int rowsAt = block.add(rows), wordsAt = block.add(words);
    StagePass pass(s, st, block);
    if (pass.begin()) return -1;
    const int H = stage_history(s->g.Z);
    if (tiles.nTiles > 0) {
        StageResArgs A;
        A.in = in.data; A.rows = pass.stage.device<StageResRow>(rowsAt);
        A.tile = tile_out(pass.stage, wordsAt, tiles, rowStride, deviceOut);
        A.hT = s->dTable.ptr; A.hist = s->dHist[s->cur].ptr;
        A.up = s->g.up; A.down = s->g.down; A.Z = s->g.Z; A.span = res_span(s->res);
        void (*const kernels[2][2])(StageResArgs) = {{klatt_stage_resample<false, int16_t>, klatt_stage_resample<true, int16_t>},
                                                     {klatt_stage_resample<false, float>, klatt_stage_resample<true, float>}};
        const unsigned grid = (unsigned)std::min<long long>(tiles.nTiles, 8ll * s->b->cus);
        hipLaunchKernelGGL(kernels[in.format()][format], dim3(grid), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    // the next history, into the buffer nothing of this push reads
    const unsigned hgrid = (unsigned)std::min<long long>((s->nRows * H + 255) / 256, 4ll * s->b->cus);
    hipLaunchKernelGGL(in.format() ? klatt_stage_history<float> : klatt_stage_history<int16_t>, dim3(hgrid), dim3(256), 0, st, in.data,
                       pass.stage.device<StageResRow>(rowsAt), s->nRows, H, s->dHist[s->cur].ptr, s->dHist[s->cur ^ 1].ptr);
    HIP_TRY(hipGetLastError());
    if (pass.finish()) return -1;
    s->cur ^= 1;
    return 0;
}

static int stage_push_filter(Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, void* deviceOut, int format, long long rowStride,
                             hipStream_t st)
{
    std::vector<StageLaneRow> packed;
    std::vector<FilterGroup> groups;
    stage_lane_rows(s, in, end, sel, rowStride, packed, groups);
    StageBlock block;
    const int rowsAt = block.add(packed), groupsAt = block.add(groups), sectionsAt = block.add(s->fil.sections);
    StagePass pass(s, st, block);
    if (pass.begin()) return -1;
    StageFilterArgs A;
    A.in = in.data; A.rows = pass.stage.device<StageLaneRow>(rowsAt);
    A.sections = pass.stage.device<FilterSection>(sectionsAt);
    A.rowStride = rowStride; A.out = deviceOut; A.state = s->dFilterState.ptr;
    return launch_filter_groups(pass.stage, groups, groupsAt, in.format(), format, A) || pass.finish() ? -1 : 0;
}

static int stage_push_code(Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, long long elements, void* decodedOut, int format,
                           void* codesOut, long long rowStride, hipStream_t st)
{
    if (s->codec != kCodecAdpcm) {      // no state: the tile kernel of the whole-row export
        if (elements == 0) return 0;
        const std::vector<ResRow> rows = stage_plain_rows(s, in, sel, rowStride);
        std::vector<long long> words;
        const TileTable tiles = tile_row_table(sel.counts.data(), sel.n, kCodeTile, rowStride, kTimelineChunkLog2, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        StagePass pass(s, st, block);
        if (pass.begin()) return -1;
        CodeArgs A;
        A.in = in.data; A.rows = pass.stage.device<ResRow>(rowsAt);
        A.tile = tile_out(pass.stage, wordsAt, tiles, rowStride, decodedOut);
        A.codes = static_cast<uint8_t*>(codesOut);
        return launch_g711(pass.stage, s->codec, in.format(), format, A) || pass.finish() ? -1 : 0;
    }
    std::vector<StageLaneRow> packed;
    std::vector<FilterGroup> groups;
    stage_lane_rows(s, in, end, sel, rowStride, packed, groups);
    StageBlock block;
    const int rowsAt = block.add(packed), groupsAt = block.add(groups);
    StagePass pass(s, st, block);
    if (pass.begin()) return -1;
    StageAdpcmArgs A;
    A.in = in.data; A.rows = pass.stage.device<StageLaneRow>(rowsAt);
    A.groups = pass.stage.device<FilterGroup>(groupsAt); A.nGroups = (long long)groups.size();
    A.rowStride = rowStride; A.decoded = decodedOut; A.codes = static_cast<uint8_t*>(codesOut); A.state = s->dCodeState.ptr;
    // Nothing to write: the codes' kernel, which then only moves the states
    const int outputs = elements == 0 ? kCodeCodes : (decodedOut ? kCodeDecoded : 0) | (codesOut ? kCodeCodes : 0);
    return launch_adpcm(pass.stage, in.format(), outputs, format, A) || pass.finish() ? -1 : 0;
}

static int stage_push_convolve(Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, void* deviceOut, int format, long long rowStride,
                               hipStream_t st)
{
    const std::vector<StageHistRow> rows = stage_history_rows(s, in, end, sel, rowStride);
    std::vector<long long> words;
    const TileTable tiles = tile_row_table(sel.counts.data(), sel.n, kConvolveTile, rowStride, kTimelineChunkLog2, words);
    StageBlock block;
    const int rowsAt = block.add(rows), wordsAt = block.add(words);
    StagePass pass(s, st, block);
    if (pass.begin()) return -1;
    if (tiles.nTiles > 0) {
        StageConvArgs A;
        A.in = in.data; A.rows = pass.stage.device<StageHistRow>(rowsAt);
        A.tile = tile_out(pass.stage, wordsAt, tiles, rowStride, deviceOut);
        A.taps = s->dTaps.ptr; A.hist = s->dHist[s->cur].ptr;
        void (*const kernels[2][2])(StageConvArgs) = {{klatt_stage_convolve<false, int16_t>, klatt_stage_convolve<true, int16_t>},
                                                      {klatt_stage_convolve<false, float>, klatt_stage_convolve<true, float>}};
        if (queue_tiles(pass.stage, kernels[in.format()][0], kernels[in.format()][1], format, kConvolveGroupsPerCu, A)) return -1;
    }
    return stage_history_finish(s, pass, in, pass.stage.device<StageHistRow>(rowsAt));
}

// A push onto a stage on the step grid -- the spectrogram, LPC, the pitch --: one staging of the rows and of the push's step table, the
// kind's kernel over the steps (its whole-row kernel's grid and dynamic LDS), then the next history
static int stage_push_frames(Stage* s, const ExportInput& in, const unsigned char* end, const ExportSelection& sel, long long elements, void* deviceOut, int format,
                             long long rowStride, hipStream_t st)
{
    const std::vector<StageHistRow> rows = stage_history_rows(s, in, end, sel, rowStride);
    const bool packed = rowStride == 0;
    std::vector<long long> words;
    const RowTable table = packed ? packed_row_table(sel.counts.data(), 0, sel.n, kTimelineChunkLog2, words) : RowTable{0, 0};
    StageBlock block;
    const int rowsAt = block.add(rows), wordsAt = block.add(words);
    void (*const specKernels[2][2])(StageSpecArgs) = {{klatt_stage_spectrogram<false, int16_t>, klatt_stage_spectrogram<true, int16_t>},
                                                      {klatt_stage_spectrogram<false, float>, klatt_stage_spectrogram<true, float>}};
    void (*const lpcKernels[2][2])(StageLpcArgs) = {{klatt_stage_lpc<false, int16_t>, klatt_stage_lpc<true, int16_t>}, {klatt_stage_lpc<false, float>, klatt_stage_lpc<true, float>}};
    void (*const pitchKernels[2][2])(StagePitchArgs) = {{klatt_stage_pitch<false, int16_t>, klatt_stage_pitch<true, int16_t>},
                                                        {klatt_stage_pitch<false, float>, klatt_stage_pitch<true, float>}};
    const auto specKernel = specKernels[in.format()][format];
    const auto lpcKernel = lpcKernels[in.format()][format];
    const auto pitchKernel = pitchKernels[in.format()][format];
    const int kind = s->g.kind;
    const void* const kernel = kind == kStageSpectrogram ? reinterpret_cast<const void*>(specKernel)
                               : kind == kStageLpc       ? reinterpret_cast<const void*>(lpcKernel)
                                                         : reinterpret_cast<const void*>(pitchKernel);
    const int budget = kind == kStageSpectrogram ? (int)kSpecLdsBudget : kind == kStageLpc ? (int)kLpcLdsBudget : (int)kPitchLdsBudget;
    StagePass pass(s, st, block);
    if (pass.begin([&] { return ensure_lds_limit(kernel, budget); })) return -1;
    if (elements > 0) {
        const StageHistRow* dRows = pass.stage.device<StageHistRow>(rowsAt);
        const long long* start = packed ? pass.stage.device<long long>(wordsAt) + table.startOff : nullptr;
        const long long* chunk = packed ? pass.stage.device<long long>(wordsAt) + table.chunkOff : nullptr;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (kind == kStageSpectrogram) {
            StageSpecArgs A;
            A.s = spec_args(pass.stage, s->spec, packed ? &table : nullptr, wordsAt, rowStride, elements, s->g.frames.hop, s->g.frames.phase, deviceOut);
            A.s.in = in.data; A.s.rows = nullptr;
            A.s.window = s->dWindow.ptr; A.s.tw = s->dTw.ptr; A.s.weights = s->dWeights.ptr; A.s.range = s->dRange.ptr;
            A.rows = dRows; A.hist = s->dHist[s->cur].ptr;
            if (queue_spectrogram(pass.stage, specKernel, A, A.s)) return -1;
        } else if (kind == kStageLpc) {
            const LpcPlan& P = s->lpc;
            StageLpcArgs A;
            A.s.in = in.data; A.s.rows = nullptr; A.s.start = start; A.s.chunk = chunk;
            A.s.rowStride = rowStride; A.s.nSteps = elements / P.nCols;
            A.s.hop = s->g.frames.hop; A.s.phase = s->g.frames.phase;
            A.s.window = s->dWindow.ptr; A.s.lag = P.hasLag ? s->dLag.ptr : nullptr;
            A.s.order = P.order; A.s.nWin = P.nWin; A.s.what = P.what; A.s.nCols = P.nCols;
            A.s.out = deviceOut;
            A.rows = dRows; A.hist = s->dHist[s->cur].ptr;
            const long long nGroups = (A.s.nSteps + kLpcGroup - 1) / kLpcGroup;
            const unsigned grid = (unsigned)std::min<long long>(nGroups, 8ll * s->b->cus);
            hipLaunchKernelGGL(lpcKernel, dim3(grid), dim3(256), lpc_lds_bytes(P.nWin, P.order, P.nCols, (int)elSize), pass.stage.st, A);
            HIP_TRY(hipGetLastError());
        } else {
            const PitchPlan& P = s->pitch;
            StagePitchArgs A;
            A.s.in = in.data; A.s.rows = nullptr; A.s.start = start; A.s.chunk = chunk;
            A.s.rowStride = rowStride; A.s.nSteps = elements / P.nCols;
            A.s.hop = s->g.frames.hop; A.s.phase = s->g.frames.phase; A.s.threshold = P.threshold;
            A.s.nWin = P.nWin; A.s.lagMin = P.lagMin; A.s.lagMax = P.lagMax; A.s.what = P.what; A.s.nCols = P.nCols; A.s.sampleRate = P.sampleRate;
            A.s.out = deviceOut;
            A.rows = dRows; A.hist = s->dHist[s->cur].ptr;
            const long long nGroups = (A.s.nSteps + kPitchGroup - 1) / kPitchGroup;
            const unsigned grid = (unsigned)std::min<long long>(nGroups, 8ll * s->b->cus);
            hipLaunchKernelGGL(pitchKernel, dim3(grid), dim3(256), pitch_lds_bytes(P.nWin, P.lagMax, P.nCols, (int)elSize), pass.stage.st, A);
            HIP_TRY(hipGetLastError());
        }
    }
    return stage_history_finish(s, pass, in, pass.stage.device<StageHistRow>(rowsAt));
}

long long speechPlayer_stage_push(speechPlayer_stage_t stage, const speechPlayer_signal_t* chunk, const unsigned char* end, void* deviceOut, int format,
                                  void* deviceCodes, long long rowStride, long long* outLengths, void* stream)
{
    const char* what = "stage_push";
    if (refuse_timing_only("speechPlayer_stage_push")) return -1;
    begin_call();
    Stage* s = stage_of(what, stage);
    if (!s) return -1;
    Batch* b = s->b;
    try {
        const bool code = s->g.kind == kStageCode, spec = stage_has_frames(s->g.kind);      // spec: the output is [step][nCols]
        const int nCols = s->g.kind == kStageSpectrogram ? s->spec.nOut : s->g.kind == kStageLpc ? s->lpc.nCols : s->g.kind == kStagePitch ? s->pitch.nCols : 1;
        if (spec) {      // (the spectrogram export's formats, rowStride in steps)
            if (format != 0 && format != 1) { set_error("%s: format %d (0 float64, 1 float32)", what, format); return -1; }
            if (rowStride < 0) { set_error("%s: rowStride %lld", what, rowStride); return -1; }
        } else if (tile_request(what, format, rowStride)) return -1;
        if (!code && deviceCodes) { set_error("%s: deviceCodes on a stage that is not a code stage", what); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, true, chunk, sig, in)) return -1;
        if (sig.nRows != s->nRows) { set_error("%s: a chunk of %lld rows for a stage of %lld", what, sig.nRows, s->nRows); return -1; }
        ExportSelection sel;
        if (stage_selection(what, s, [&](long long i) { return sig.len(i); }, end, sel)) return -1;
        bool active = false;      // a row that is neither fed nor ended is untouched
        for (long long i = 0; i < s->nRows && !active; ++i) active = sig.len(i) > 0 || (end && end[i]);
        static constexpr ExportNouns kBandNouns{"largest step count", "steps", "bands"};
        static constexpr ExportNouns kFieldNouns{"largest step count", "steps", "values"};
        const long long elements = spec ? export_elements(what, s->g.kind == kStageSpectrogram ? kBandNouns : kFieldNouns, sel, rowStride, nCols)
                                        : export_elements(what, kSampleNouns, sel, rowStride, 1);
        if (elements < 0) return -1;
        if (code && elements > 0 && !deviceOut && !deviceCodes) { set_error("%s: no output (the decoded samples, the codes or both)", what); return -1; }
        if (elements > 0 || active) {
            HIP_TRY(hipSetDevice(b->device));
            const size_t elSize = format ? sizeof(float) : spec ? sizeof(double) : sizeof(int16_t);
            if (elements > 0) {
                if ((!code || deviceOut) && export_output(b, what, deviceOut, elements, elSize)) return -1;
                if (deviceCodes && export_output(b, what, deviceCodes, elements, 1)) return -1;
                if (deviceOut && deviceCodes) {
                    const uintptr_t d = reinterpret_cast<uintptr_t>(deviceOut), c = reinterpret_cast<uintptr_t>(deviceCodes);
                    if (d < c + (size_t)elements && c < d + (size_t)elements * elSize) { set_error("%s: the decoded samples and the codes overlap", what); return -1; }
                }
            }
            if (signal_memory(in, what, deviceOut, deviceOut ? (size_t)elements * elSize : 0) || (deviceCodes && signal_memory(in, what, deviceCodes, (size_t)elements))) return -1;
            hipStream_t st = static_cast<hipStream_t>(stream);
            const int rc = s->g.kind == kStageResample ? stage_push_resample(s, in, end, sel, elements, deviceOut, format, rowStride, st)
                         : s->g.kind == kStageFilter   ? stage_push_filter(s, in, end, sel, deviceOut, format, rowStride, st)
                         : s->g.kind == kStageConvolve ? stage_push_convolve(s, in, end, sel, deviceOut, format, rowStride, st)
                         : spec                        ? stage_push_frames(s, in, end, sel, elements, deviceOut, format, rowStride, st)
                                                       : stage_push_code(s, in, end, sel, elements, deviceOut, format, deviceCodes, rowStride, st);
            if (rc) return -1;
        }
        for (long long i = 0; i < s->nRows; ++i) {
            stage_row_advance(s->N[(size_t)i], s->M[(size_t)i], sig.len(i), end && end[i], sel.counts[(size_t)i]);
            if (outLengths) outLengths[i] = sel.counts[(size_t)i];
        }
        return elements;
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

// The chosen rows (NULL: all) are fresh again: N = M = 0 and their state +0, behind the stage's last push
int speechPlayer_stage_reset(speechPlayer_stage_t stage, const unsigned char* rows, void* stream)
{
    begin_call();
    const char* what = "stage_reset";
    Stage* s = stage_of(what, stage);
    if (!s) return -1;
    try {
        uint32_t* state = nullptr;      // the lane state of a filter or an ADPCM stage
        int perRow = 0;
        if (s->g.kind == kStageFilter) { state = reinterpret_cast<uint32_t*>(s->dFilterState.ptr); perRow = kStageFilterState; }
        else if (s->g.kind == kStageCode && s->codec == kCodecAdpcm) { state = reinterpret_cast<uint32_t*>(s->dCodeState.ptr); perRow = 2; }
        if (stage_keeps_history(s->g.kind) && s->mostHistory > 0) {      // a history per row, each from its own first element
            HIP_TRY(hipSetDevice(s->b->device));
            StageBlock block;
            const int rowsAt = rows ? block.add(rows, (size_t)s->nRows) : -1, atAt = block.add(s->histAt);
            StagePass pass(s, static_cast<hipStream_t>(stream), block);
            if (pass.begin()) return -1;
            const dim3 grid((unsigned)std::min<long long>((s->mostHistory + 255) / 256, 64), (unsigned)std::min<long long>(s->nRows, 16ll * s->b->cus));
            hipLaunchKernelGGL(klatt_stage_clear_rows, grid, dim3(256), 0, pass.stage.st, rows ? pass.stage.device<unsigned char>(rowsAt) : nullptr,
                               pass.stage.device<long long>(atAt), s->nRows, s->dHist[s->cur].ptr);
            HIP_TRY(hipGetLastError());
            if (pass.finish()) return -1;
        }
        if (state) {
            HIP_TRY(hipSetDevice(s->b->device));
            StageBlock block;
            const int rowsAt = rows ? block.add(rows, (size_t)s->nRows) : -1;
            StagePass pass(s, static_cast<hipStream_t>(stream), block);
            if (pass.begin()) return -1;
            const long long cells = s->nRows * perRow;
            const unsigned grid = (unsigned)std::min<long long>((cells + 255) / 256, 4ll * s->b->cus);
            hipLaunchKernelGGL(klatt_stage_clear, dim3(grid), dim3(256), 0, pass.stage.st, rows ? pass.stage.device<unsigned char>(rowsAt) : nullptr, s->nRows, perRow, state);
            HIP_TRY(hipGetLastError());
            if (pass.finish()) return -1;
        }
        for (long long i = 0; i < s->nRows; ++i)
            if (!rows || rows[i]) { s->N[(size_t)i] = 0; s->M[(size_t)i] = 0; }
        return 0;
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

// Host only: the samples every row has consumed and the outputs it has emitted since its start; either may be NULL
int speechPlayer_stage_counts(speechPlayer_stage_t stage, long long* consumed, long long* emitted)
{
    begin_call();
    Stage* s = stage_of("stage_counts", stage);
    if (!s) return -1;
    for (long long i = 0; i < s->nRows; ++i) {
        if (consumed) consumed[i] = s->N[(size_t)i];
        if (emitted) emitted[i] = s->M[(size_t)i];
    }
    return 0;
}

void speechPlayer_stage_free(speechPlayer_stage_t stage)
{
    begin_call();
    Stage* s = static_cast<Stage*>(stage);
    if (s && stage_known(s)) stage_release(s);
}

// ---- linear prediction of the PCM (klatt_lpc.h) -------------------------------------------------------------------------------------------
// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernels are compiled from.
long long speechPlayer_lpcFromAutocorrelation(const double* r, int order, double* a, double* k, double* error, int* stages)
{
    begin_call();
    const char* what = "lpcFromAutocorrelation";
    if (order < 1 || order > kLpcMaxOrder) { set_error("%s: order %d (1 .. %d)", what, order, kLpcMaxOrder); return -1; }
    if (!r) { set_error("%s: no autocorrelation (order + 1 values)", what); return -1; }
    double rr[kLpcMaxOrder + 1] = {}, aa[kLpcMaxOrder + 1], kk[kLpcMaxOrder + 1], E;
    int done;
    for (int i = 0; i <= order; ++i) rr[i] = r[i];
    lpc_levinson(rr, order, aa, kk, E, done);
    for (int i = 1; i <= order; ++i) { if (a) a[i - 1] = aa[i]; if (k) k[i - 1] = kk[i]; }
    if (error) *error = E;
    if (stages) *stages = done;
    return order;
}

static long long lpc_statement(const char* what, const void* x, int inFormat, long long length, int order, int nWin, long long hop, long long phase,
                               const double* window, const double* lagWindow, int fields, double* out)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || hop <= 0 || phase < 0 || (length > 0 && !x)) {
        set_error("%s: length %lld (0 .. 2^44, with its samples), hop %lld, phase %lld", what, length, hop, phase); return -1;
    }
    try {
        LpcPlan P;
        std::string why;
        if (!lpc_plan(P, order, nWin, window, lagWindow, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
        if (align_steps_below(length, hop, phase) > 0 && !out) { set_error("%s: no output", what); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? lpc_host(static_cast<const float*>(x), length, P, hop, phase, out) : lpc_host(static_cast<const int16_t*>(x), length, P, hop, phase, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmLpc(const sample* pcm, long long length, int order, int nWin, long long hop, long long phase, const double* window,
                              const double* lagWindow, int what, double* out)
{
    begin_call();
    return lpc_statement("pcmLpc", pcm, 0, length, order, nWin, hop, phase, window, lagWindow, what, out);
}

long long speechPlayer_signalLpc(const void* x, int inFormat, long long length, int order, int nWin, long long hop, long long phase, const double* window,
                                 const double* lagWindow, int what, double* out)
{
    begin_call();
    return lpc_statement("signalLpc", x, inFormat, length, order, nWin, hop, phase, window, lagWindow, what, out);
}

// What the inverse filter's statements and exports share of their request
static int lpc_residual_request(const char* what, int order, int which, int format)
{
    if (order < 1 || order > kLpcMaxOrder) { set_error("%s: order %d (1 .. %d)", what, order, kLpcMaxOrder); return -1; }
    if (which != kLpcResidual && which != kLpcPrediction) { set_error("%s: what %d (0 residual, 1 prediction)", what, which); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    return 0;
}

static long long lpc_residual_statement(const char* what, const void* x, int inFormat, long long length, int order, long long hop, long long phase,
                                        const double* coeff, int which, int format, void* out, long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || hop <= 0 || phase < 0 || (length > 0 && !x)) {
        set_error("%s: length %lld (0 .. 2^44, with its samples), hop %lld, phase %lld", what, length, hop, phase); return -1;
    }
    if (lpc_residual_request(what, order, which, format)) return -1;
    hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
    if (align_steps_below(length, hop, phase) > 0 && !coeff) { set_error("%s: no coefficients ([steps][order] doubles)", what); return -1; }
    if (length > 0 && !out) { set_error("%s: no output", what); return -1; }
    if (capacity < length) { set_error("%s: the output takes %lld elements, capacity is %lld", what, length, capacity); return -1; }
    if (signal_host_values(what, x, inFormat, length)) return -1;
    if (inFormat) lpc_inverse_host(static_cast<const float*>(x), length, order, hop, phase, coeff, which, format, out);
    else lpc_inverse_host(static_cast<const int16_t*>(x), length, order, hop, phase, coeff, which, format, out);
    return length;
}

long long speechPlayer_pcmLpcResidual(const sample* pcm, long long length, int order, long long hop, long long phase, const double* coeff, int what, int format,
                                      void* out, long long capacity)
{
    begin_call();
    return lpc_residual_statement("pcmLpcResidual", pcm, 0, length, order, hop, phase, coeff, what, format, out, capacity);
}

long long speechPlayer_signalLpcResidual(const void* x, int inFormat, long long length, int order, long long hop, long long phase, const double* coeff, int what,
                                         int format, void* out, long long capacity)
{
    begin_call();
    return lpc_residual_statement("signalLpcResidual", x, inFormat, length, order, hop, phase, coeff, what, format, out, capacity);
}

// The analysis of chosen utterances' PCM, 64 steps of the output per workgroup (klatt_lpc.h).  The host path is spectrogram_export's, step for
// step: it reads the pool, so it is ordered as speechPlayer_batch_exportPcm is (ExportStage, ofPcm).  The staging block: rows | step starts
// and chunk rows (packed) | window | lag window.  ofSignal and `signal` as spectrogram_export's.
static long long lpc_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances,
                            int order, int nWin, long long hop, long long phase, const double* window, const double* lagWindow, int fields, void* deviceOut, int format,
                            long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("%s: format %d (0 float64, 1 float32)", what, format); return -1; }
        if (step_request(what, hop, phase, rowStride)) return -1;
        LpcPlan P;
        std::string why;
        if (!lpc_plan(P, order, nWin, window, lagWindow, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<SpecRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long, long long u, long long) {
                const long long L = in.len(u);
                rows.push_back(SpecRow{in.at(u), L, align_steps_below(L, hop, phase)});
                return rows.back().steps;
            }, in.sig)) return -1;
        static constexpr ExportNouns kFieldNouns{"largest step count", "steps", "values"};
        const long long elements = export_elements(what, kFieldNouns, s, rowStride, P.nCols);
        if (elements <= 0) return elements;
        if (!in.sig && export_synthesised(b, what)) return -1;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize) || signal_memory(in, what, deviceOut, (size_t)elements * elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        const bool packed = rowStride == 0;
        std::vector<long long> words;
        const RowTable table = packed ? packed_row_table(s.counts.data(), 0, s.n, kTimelineChunkLog2, words) : RowTable{0, 0};
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), windowAt = block.add(P.window), lagAt = block.add(P.lag);
        void (*const kernels[2][2])(LpcArgs) = {{klatt_lpc<false, int16_t>, klatt_lpc<true, int16_t>}, {klatt_lpc<false, float>, klatt_lpc<true, float>}};
        const auto kernel = kernels[in.format()][format];
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin([&] { return ensure_lds_limit(reinterpret_cast<const void*>(kernel), (int)kLpcLdsBudget); })) return -1;
        LpcArgs A;
        A.in = in.data; A.rows = stage.device<SpecRow>(rowsAt);
        A.start = packed ? stage.device<long long>(wordsAt) + table.startOff : nullptr;
        A.chunk = packed ? stage.device<long long>(wordsAt) + table.chunkOff : nullptr;
        A.rowStride = rowStride; A.nSteps = elements / P.nCols;
        A.hop = hop; A.phase = phase;
        A.window = stage.device<float>(windowAt); A.lag = P.hasLag ? stage.device<double>(lagAt) : nullptr;
        A.order = P.order; A.nWin = P.nWin; A.what = P.what; A.nCols = P.nCols;
        A.out = deviceOut;
        const long long nGroups = (A.nSteps + kLpcGroup - 1) / kLpcGroup;
        const unsigned grid = (unsigned)std::min<long long>(nGroups, 8ll * b->cus);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lpc_lds_bytes(P.nWin, P.order, P.nCols, (int)elSize), st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportLpc(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, int nWin, long long hop,
                                       long long phase, const double* window, const double* lagWindow, int what, void* deviceOut, int format, long long rowStride,
                                       void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpc")) return -1;
    return lpc_export("exportLpc", batch, false, nullptr, utterances, nUtterances, order, nWin, hop, phase, window, lagWindow, what, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportLpcOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int order, int nWin,
                                         long long hop, long long phase, const double* window, const double* lagWindow, int what, void* deviceOut, int format,
                                         long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpcOf")) return -1;
    return lpc_export("exportLpcOf", batch, true, signal, rows, nRows, order, nWin, hop, phase, window, lagWindow, what, deviceOut, format, rowStride, stream);
}

// ---- pitch estimated from the PCM (klatt_pitch.h) ---------------------------------------------------------------------------------------------
// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernel is compiled from.
static long long pitch_statement(const char* what, const void* x, int inFormat, long long length, int sampleRate, int nWin, int lagMin, int lagMax,
                                 double threshold, long long hop, long long phase, int fields, double* out)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || hop <= 0 || phase < 0 || (length > 0 && !x)) {
        set_error("%s: length %lld (0 .. 2^44, with its samples), hop %lld, phase %lld", what, length, hop, phase); return -1;
    }
    try {
        PitchPlan P;
        std::string why;
        if (!pitch_plan(P, sampleRate, nWin, lagMin, lagMax, threshold, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
        if (align_steps_below(length, hop, phase) > 0 && !out) { set_error("%s: no output", what); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        return inFormat ? pitch_host(static_cast<const float*>(x), length, P, hop, phase, out) : pitch_host(static_cast<const int16_t*>(x), length, P, hop, phase, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmPitch(const sample* pcm, long long length, int sampleRate, int nWin, int lagMin, int lagMax, double threshold, long long hop,
                                long long phase, int what, double* out)
{
    begin_call();
    return pitch_statement("pcmPitch", pcm, 0, length, sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, what, out);
}

long long speechPlayer_signalPitch(const void* x, int inFormat, long long length, int sampleRate, int nWin, int lagMin, int lagMax, double threshold,
                                   long long hop, long long phase, int what, double* out)
{
    begin_call();
    return pitch_statement("signalPitch", x, inFormat, length, sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, what, out);
}

// The pitch of chosen utterances' PCM, 16 steps of the output per workgroup, four per wavefront (klatt_pitch.h).  The host path is lpc_export's,
// step for step.  The staging block: rows | step starts and chunk rows (packed).  ofSignal and `signal` as spectrogram_export's.
static long long pitch_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances,
                              long long nUtterances, int sampleRate, int nWin, int lagMin, int lagMax, double threshold, long long hop, long long phase, int fields,
                              void* deviceOut, int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (format != 0 && format != 1) { set_error("%s: format %d (0 float64, 1 float32)", what, format); return -1; }
        if (step_request(what, hop, phase, rowStride)) return -1;
        PitchPlan P;
        std::string why;
        if (!pitch_plan(P, ofSignal ? sampleRate : b->sampleRate, nWin, lagMin, lagMax, threshold, fields, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<SpecRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long, long long u, long long) {
                const long long L = in.len(u);
                rows.push_back(SpecRow{in.at(u), L, align_steps_below(L, hop, phase)});
                return rows.back().steps;
            }, in.sig)) return -1;
        static constexpr ExportNouns kFieldNouns{"largest step count", "steps", "values"};
        const long long elements = export_elements(what, kFieldNouns, s, rowStride, P.nCols);
        if (elements <= 0) return elements;
        if (!in.sig && export_synthesised(b, what)) return -1;
        const size_t elSize = format ? sizeof(float) : sizeof(double);
        if (export_output(b, what, deviceOut, elements, elSize) || signal_memory(in, what, deviceOut, (size_t)elements * elSize)) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        const bool packed = rowStride == 0;
        std::vector<long long> words;
        const RowTable table = packed ? packed_row_table(s.counts.data(), 0, s.n, kTimelineChunkLog2, words) : RowTable{0, 0};
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        void (*const kernels[2][2])(PitchArgs) = {{klatt_pitch<false, int16_t>, klatt_pitch<true, int16_t>}, {klatt_pitch<false, float>, klatt_pitch<true, float>}};
        const auto kernel = kernels[in.format()][format];
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin([&] { return ensure_lds_limit(reinterpret_cast<const void*>(kernel), (int)kPitchLdsBudget); })) return -1;
        PitchArgs A;
        A.in = in.data; A.rows = stage.device<SpecRow>(rowsAt);
        A.start = packed ? stage.device<long long>(wordsAt) + table.startOff : nullptr;
        A.chunk = packed ? stage.device<long long>(wordsAt) + table.chunkOff : nullptr;
        A.rowStride = rowStride; A.nSteps = elements / P.nCols;
        A.hop = hop; A.phase = phase; A.threshold = P.threshold;
        A.nWin = P.nWin; A.lagMin = P.lagMin; A.lagMax = P.lagMax; A.what = P.what; A.nCols = P.nCols; A.sampleRate = P.sampleRate;
        A.out = deviceOut;
        const long long nGroups = (A.nSteps + kPitchGroup - 1) / kPitchGroup;
        const unsigned grid = (unsigned)std::min<long long>(nGroups, 8ll * b->cus);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), pitch_lds_bytes(P.nWin, P.lagMax, P.nCols, (int)elSize), st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportPitch(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int nWin, int lagMin, int lagMax,
                                         double threshold, long long hop, long long phase, int what, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportPitch")) return -1;
    return pitch_export("exportPitch", batch, false, nullptr, utterances, nUtterances, 0, nWin, lagMin, lagMax, threshold, hop, phase, what, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal at `sampleRate`: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportPitchOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int sampleRate,
                                           int nWin, int lagMin, int lagMax, double threshold, long long hop, long long phase, int what, void* deviceOut, int format,
                                           long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportPitchOf")) return -1;
    return pitch_export("exportPitchOf", batch, true, signal, rows, nRows, sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, what, deviceOut, format, rowStride, stream);
}

// The chosen rows through the inverse filter of their own frames' coefficients, tile-wise (klatt_lpc.h): the residual or the prediction.  The
// host path is the tile-wise exports'; the coefficients are a device tensor [row][step][coeffCols], checked as the signal's memory is.  The
// staging block: rows | tile starts and chunk rows (packed).  Nothing is kept on the batch.  ofSignal and `signal` as spectrogram_export's.
static long long lpc_residual_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances,
                                     long long nUtterances, int order, long long hop, long long phase, const void* coeff, int coeffFormat, int coeffCols, int col0,
                                     long long coeffStride, int which, void* deviceOut, int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        if (lpc_residual_request(what, order, which, format)) return -1;
        if (hop <= 0 || phase < 0) { set_error("%s: hop %lld, phase %lld", what, hop, phase); return -1; }
        hop = std::min(hop, 1ll << 40); phase = std::min(phase, 1ll << 40);
        if (coeffFormat != 0 && coeffFormat != 1) { set_error("%s: coefficient format %d (0 float64, 1 float32)", what, coeffFormat); return -1; }
        if (coeffCols < 1 || coeffCols > (1 << 20) || col0 < 0 || col0 > coeffCols - order) {
            set_error("%s: coefficients a_1 .. a_%d at columns %d .. %d of %d (1 .. 2^20)", what, order, col0, col0 + order - 1, coeffCols); return -1;
        }
        if (coeffStride < 0) { set_error("%s: coeffStride %lld", what, coeffStride); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<LpcResRow> rows;
        long long stepsBefore = 0, mostSteps = 0;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) {
                const long long L = in.len(u), steps = align_steps_below(L, hop, phase);
                rows.push_back(LpcResRow{in.at(u), L, steps, tile_row_first(i, rowStride, before), tile_row_first(i, coeffStride, stepsBefore)});      // (the extent below refuses a stride that wraps)
                stepsBefore += steps; mostSteps = std::max(mostSteps, steps);
                return L;
            }, in.sig)) return -1;
        if (coeffStride > 0 && coeffStride < mostSteps) { set_error("%s: coeffStride %lld is below the largest step count (%lld)", what, coeffStride, mostSteps); return -1; }
        // the coefficients' extent, by division before any product (as export_extent's): rows without steps read none
        const long long coeffLimit = kExportLimit / coeffCols;
        if (coeffStride > 0 && mostSteps > 0 && s.n > coeffLimit / coeffStride) {
            set_error("%s: %lld rows of coeffStride %lld steps of %d coefficient columns (at most 2^50 elements)", what, s.n, coeffStride, coeffCols); return -1;
        }
        const long long coeffSteps = coeffStride > 0 ? (mostSteps > 0 ? s.n * coeffStride : 0) : stepsBefore;
        if (coeffSteps > coeffLimit) { set_error("%s: %lld steps of %d coefficient columns (at most 2^50 elements)", what, coeffSteps, coeffCols); return -1; }
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(int16_t), cSize = coeffFormat ? sizeof(float) : sizeof(double);
        const size_t outBytes = (size_t)elements * elSize, coeffBytes = (size_t)coeffSteps * (size_t)coeffCols * cSize;
        if (coeffBytes) {
            if (!coeff) { set_error("%s: no coefficients", what); return -1; }
            const std::string name = std::string(what) + ": coefficients";
            if (!device_range(coeff, coeffBytes, b->device, cSize, name.c_str())) return -1;
            const uintptr_t c = reinterpret_cast<uintptr_t>(coeff), o = reinterpret_cast<uintptr_t>(deviceOut);
            if (c < o + outBytes && o < c + coeffBytes) {
                set_error("%s: the output (%zu bytes from %p) overlaps the coefficients (%zu bytes from %p)", what, outBytes, deviceOut, coeffBytes, coeff); return -1;
            }
        }
        hipStream_t st = static_cast<hipStream_t>(stream);
        std::vector<long long> words;
        const TileTable tiles = tile_row_table(s.counts.data(), s.n, kLpcTile, rowStride, kTimelineChunkLog2, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words);
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        LpcResArgs A;
        A.in = in.data; A.rows = stage.device<LpcResRow>(rowsAt);
        A.tile = tile_out(stage, wordsAt, tiles, rowStride, deviceOut);
        A.coeff = coeff; A.hop = hop; A.phase = phase;
        A.order = order; A.coeffCols = coeffCols; A.col0 = col0;
        constexpr int R = kLpcResidual, Q = kLpcPrediction;
        // [what][coefficient format][input format][output format]
        void (*const kernels[2][2][2][2])(LpcResArgs) = {
            {{{klatt_lpc_residual<R, false, int16_t, false>, klatt_lpc_residual<R, true, int16_t, false>}, {klatt_lpc_residual<R, false, float, false>, klatt_lpc_residual<R, true, float, false>}},
             {{klatt_lpc_residual<R, false, int16_t, true>, klatt_lpc_residual<R, true, int16_t, true>}, {klatt_lpc_residual<R, false, float, true>, klatt_lpc_residual<R, true, float, true>}}},
            {{{klatt_lpc_residual<Q, false, int16_t, false>, klatt_lpc_residual<Q, true, int16_t, false>}, {klatt_lpc_residual<Q, false, float, false>, klatt_lpc_residual<Q, true, float, false>}},
             {{klatt_lpc_residual<Q, false, int16_t, true>, klatt_lpc_residual<Q, true, int16_t, true>}, {klatt_lpc_residual<Q, false, float, true>, klatt_lpc_residual<Q, true, float, true>}}}};
        if (launch_tiles(stage, kernels[which][coeffFormat], in.format(), format, 8, A)) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportLpcResidual(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, long long hop, long long phase,
                                               const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride, int what, void* deviceOut,
                                               int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpcResidual")) return -1;
    return lpc_residual_export("exportLpcResidual", batch, false, nullptr, utterances, nUtterances, order, hop, phase, deviceCoeff, coeffFormat, coeffCols, col0, coeffStride,
                               what, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportLpcResidualOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int order,
                                                 long long hop, long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride,
                                                 int what, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpcResidualOf")) return -1;
    return lpc_residual_export("exportLpcResidualOf", batch, true, signal, rows, nRows, order, hop, phase, deviceCoeff, coeffFormat, coeffCols, col0, coeffStride, what,
                               deviceOut, format, rowStride, stream);
}

// ---- LPC synthesis: an excitation through 1 / A(z) (klatt_lpcsynth.h) ---------------------------------------------------------------------------
static_assert(sizeof(LpcSynthRow) == sizeof(FilterRow) + 16 && sizeof(LpcSynthRow) % 8 == 0, "a row is an array of 8-byte words: a FilterRow, its first coefficient step, its steps");

// Host only, touches no device: the step-up recursion, lpc_levinson's update of a[] with the reflection coefficients given.
long long speechPlayer_lpcFromReflection(const double* k, int order, double* a)
{
    begin_call();
    const char* what = "lpcFromReflection";
    if (order < 1 || order > kLpcMaxOrder) { set_error("%s: order %d (1 .. %d)", what, order, kLpcMaxOrder); return -1; }
    if (!k || !a) { set_error("%s: no %s (order values)", what, k ? "output" : "reflection coefficients"); return -1; }
    double kk[kLpcMaxOrder + 1] = {}, aa[kLpcMaxOrder + 1];
    for (int i = 1; i <= order; ++i) kk[i] = k[i - 1];
    lpc_step_up(kk, order, aa);
    for (int i = 1; i <= order; ++i) a[i - 1] = aa[i];
    return order;
}

// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernel is compiled from.
static long long lpc_synth_statement(const char* what, const void* x, int inFormat, long long length, int order, long long hop, long long phase,
                                     const double* coeff, int format, void* out, long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kResampleMaxLength || hop <= 0 || phase < 0 || (length > 0 && !x)) {
        set_error("%s: length %lld (0 .. 2^44, with its samples), hop %lld, phase %lld", what, length, hop, phase); return -1;
    }
    LpcSynthPlan P;
    std::string why;
    if (!lpc_synth_plan(P, order, hop, phase, format, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
    if (align_steps_below(length, P.hop, P.phase) > 0 && !coeff) { set_error("%s: no coefficients ([steps][order] doubles)", what); return -1; }
    if (length > 0 && !out) { set_error("%s: no output", what); return -1; }
    if (capacity < length) { set_error("%s: the output takes %lld elements, capacity is %lld", what, length, capacity); return -1; }
    if (signal_host_values(what, x, inFormat, length)) return -1;
    if (inFormat) lpc_synth_host(static_cast<const float*>(x), length, order, P.hop, P.phase, coeff, format, out);
    else lpc_synth_host(static_cast<const int16_t*>(x), length, order, P.hop, P.phase, coeff, format, out);
    return length;
}

long long speechPlayer_pcmLpcSynthesis(const sample* pcm, long long length, int order, long long hop, long long phase, const double* coeff, int format, void* out,
                                       long long capacity)
{
    begin_call();
    return lpc_synth_statement("pcmLpcSynthesis", pcm, 0, length, order, hop, phase, coeff, format, out, capacity);
}

long long speechPlayer_signalLpcSynthesis(const void* x, int inFormat, long long length, int order, long long hop, long long phase, const double* coeff, int format,
                                          void* out, long long capacity)
{
    begin_call();
    return lpc_synth_statement("signalLpcSynthesis", x, inFormat, length, order, hop, phase, coeff, format, out, capacity);
}

// klatt_lpc_synth of a ring, a coefficient format, an input format and an output format
extern "C++" template <int B>
static void (*lpc_synth_kernel(int coeffFormat, int inFormat, int format))(LpcSynthArgs)
{
    void (*const kernels[2][2][2])(LpcSynthArgs) = {
        {{klatt_lpc_synth<B, false, int16_t, false>, klatt_lpc_synth<B, true, int16_t, false>}, {klatt_lpc_synth<B, false, float, false>, klatt_lpc_synth<B, true, float, false>}},
        {{klatt_lpc_synth<B, false, int16_t, true>, klatt_lpc_synth<B, true, int16_t, true>}, {klatt_lpc_synth<B, false, float, true>, klatt_lpc_synth<B, true, float, true>}}};
    return kernels[coeffFormat][inFormat][format];
}

// The chosen rows through the recursive filter of their own frames' coefficients (klatt_lpcsynth.h).  The request, the coefficient tensor and
// its checks are lpc_residual_export's without `what`; the rows go a wavefront per 64 as filtered_export's (the staging block: packed rows |
// groups), all in one launch.  Nothing is kept on the batch.  ofSignal and `signal` as spectrogram_export's.
static long long lpc_synth_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances,
                                  long long nUtterances, int order, long long hop, long long phase, const void* coeff, int coeffFormat, int coeffCols, int col0,
                                  long long coeffStride, void* deviceOut, int format, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        LpcSynthPlan P;
        std::string why;
        if (!lpc_synth_plan(P, order, hop, phase, format, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        if (coeffFormat != 0 && coeffFormat != 1) { set_error("%s: coefficient format %d (0 float64, 1 float32)", what, coeffFormat); return -1; }
        if (coeffCols < 1 || coeffCols > (1 << 20) || col0 < 0 || col0 > coeffCols - order) {
            set_error("%s: coefficients a_1 .. a_%d at columns %d .. %d of %d (1 .. 2^20)", what, order, col0, col0 + order - 1, coeffCols); return -1;
        }
        if (coeffStride < 0) { set_error("%s: coeffStride %lld", what, coeffStride); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<LpcSynthRow> rows;
        long long stepsBefore = 0, mostSteps = 0;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) {
                const long long L = in.len(u), steps = align_steps_below(L, P.hop, P.phase);
                rows.push_back(lpc_synth_row(in.at(u), L, tile_row_first(i, rowStride, before), tile_row_first(i, coeffStride, stepsBefore), steps));      // (the extent below refuses a stride that wraps)
                stepsBefore += steps; mostSteps = std::max(mostSteps, steps);
                return L;
            }, in.sig)) return -1;
        if (coeffStride > 0 && coeffStride < mostSteps) { set_error("%s: coeffStride %lld is below the largest step count (%lld)", what, coeffStride, mostSteps); return -1; }
        // the coefficients' extent, by division before any product (as export_extent's): rows without steps read none
        const long long coeffLimit = kExportLimit / coeffCols;
        if (coeffStride > 0 && mostSteps > 0 && s.n > coeffLimit / coeffStride) {
            set_error("%s: %lld rows of coeffStride %lld steps of %d coefficient columns (at most 2^50 elements)", what, s.n, coeffStride, coeffCols); return -1;
        }
        const long long coeffSteps = coeffStride > 0 ? (mostSteps > 0 ? s.n * coeffStride : 0) : stepsBefore;
        if (coeffSteps > coeffLimit) { set_error("%s: %lld steps of %d coefficient columns (at most 2^50 elements)", what, coeffSteps, coeffCols); return -1; }
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(int16_t), cSize = coeffFormat ? sizeof(float) : sizeof(double);
        const size_t outBytes = (size_t)elements * elSize, coeffBytes = (size_t)coeffSteps * (size_t)coeffCols * cSize;
        if (coeffBytes) {
            if (!coeff) { set_error("%s: no coefficients", what); return -1; }
            const std::string name = std::string(what) + ": coefficients";
            if (!device_range(coeff, coeffBytes, b->device, cSize, name.c_str())) return -1;
            const uintptr_t c = reinterpret_cast<uintptr_t>(coeff), o = reinterpret_cast<uintptr_t>(deviceOut);
            if (c < o + outBytes && o < c + coeffBytes) {
                set_error("%s: the output (%zu bytes from %p) overlaps the coefficients (%zu bytes from %p)", what, outBytes, deviceOut, coeffBytes, coeff); return -1;
            }
        }
        std::vector<LpcSynthRow> packed;
        std::vector<FilterGroup> groups;
        lpc_synth_pack(rows, packed, groups);
        StageBlock block;
        const int rowsAt = block.add(packed), groupsAt = block.add(groups);
        ExportStage stage(b, static_cast<hipStream_t>(stream), block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        LpcSynthArgs A;
        A.in = in.data; A.rows = stage.device<LpcSynthRow>(rowsAt);
        A.groups = stage.device<FilterGroup>(groupsAt); A.nGroups = (long long)groups.size();
        A.rowStride = rowStride; A.out = deviceOut;
        A.coeff = coeff; A.hop = P.hop; A.phase = P.phase;
        A.order = order; A.coeffCols = coeffCols; A.col0 = col0;
        const auto kernel = P.history == 8 ? lpc_synth_kernel<8>(coeffFormat, in.format(), format)
                          : P.history == 16 ? lpc_synth_kernel<16>(coeffFormat, in.format(), format) : lpc_synth_kernel<32>(coeffFormat, in.format(), format);
        const unsigned grid = (unsigned)std::min<long long>(A.nGroups, 64ll * b->cus);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kFilterLanes), 0, stage.st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportLpcSynthesis(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, long long hop, long long phase,
                                                const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride, void* deviceOut, int format,
                                                long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpcSynthesis")) return -1;
    return lpc_synth_export("exportLpcSynthesis", batch, false, nullptr, utterances, nUtterances, order, hop, phase, deviceCoeff, coeffFormat, coeffCols, col0, coeffStride,
                            deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportLpcSynthesisOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, int order,
                                                  long long hop, long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride,
                                                  void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportLpcSynthesisOf")) return -1;
    return lpc_synth_export("exportLpcSynthesisOf", batch, true, signal, rows, nRows, order, hop, phase, deviceCoeff, coeffFormat, coeffCols, col0, coeffStride,
                            deviceOut, format, rowStride, stream);
}

// ---- the PCM at another tempo by WSOLA (klatt_tempo.h) ----------------------------------------------------------------------------------------
// Host only, touch no device: the definition of include/speechPlayer_batch.h through the functions the kernels are compiled from.
static int tempo_length_request(const char* what, long long length, double tempo)
{
    if (length < 0 || length > kResampleMaxLength) { set_error("%s: length %lld (0 .. 2^44)", what, length); return -1; }
    if (!tempo_valid(tempo)) { set_error("%s: tempo %g (finite, 0.25 .. 4)", what, tempo); return -1; }
    return 0;
}

long long speechPlayer_tempoLength(long long length, double tempo)
{
    begin_call();
    if (tempo_length_request("tempoLength", length, tempo)) return -1;
    return tempo_out_length(length, tempo);
}

long long speechPlayer_tempoFrames(long long length, double tempo, int nWin)
{
    begin_call();
    if (tempo_length_request("tempoFrames", length, tempo)) return -1;
    TempoPlan P;
    std::string why;
    if (!tempo_plan(P, nWin, 0, false, why)) { set_error("tempoFrames: %s", why.c_str()); return -1; }
    return tempo_frames(tempo_out_length(length, tempo), P.Hs);
}

static long long tempo_statement(const char* what, const void* x, int inFormat, long long length, double tempo, int nWin, int search, const long long* positionsIn,
                                 long long* positionsOut, int format, void* out, long long capacity)
{
    if (signal_host_format(what, inFormat)) return -1;
    if (length > 0 && !x) { set_error("%s: length %lld without samples", what, length); return -1; }
    if (tempo_length_request(what, length, tempo)) return -1;
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    try {
        TempoPlan P;
        std::string why;
        if (!tempo_plan(P, nWin, search, positionsIn == nullptr, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        const long long Lout = tempo_out_length(length, tempo), K = tempo_frames(Lout, P.Hs);
        if (out && capacity < Lout) { set_error("%s: the output takes %lld elements, capacity is %lld", what, Lout, capacity); return -1; }
        if (signal_host_values(what, x, inFormat, length)) return -1;
        std::vector<long long> own;
        const long long* p = positionsIn;
        if (!p && (out || positionsOut)) {
            own.resize((size_t)K);
            if (inFormat) tempo_positions_host(static_cast<const float*>(x), length, P, tempo, K, own.data());
            else tempo_positions_host(static_cast<const int16_t*>(x), length, P, tempo, K, own.data());
            p = own.data();
        }
        for (long long k = 0; positionsOut && k < K; ++k) positionsOut[k] = p[k];
        if (out) {
            if (inFormat) tempo_render_host(static_cast<const float*>(x), length, P, Lout, p, format, out);
            else tempo_render_host(static_cast<const int16_t*>(x), length, P, Lout, p, format, out);
        }
        return Lout;
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmTempo(const sample* pcm, long long length, double tempo, int nWin, int search, const long long* positionsIn, long long* positionsOut,
                                int format, void* out, long long capacity)
{
    begin_call();
    return tempo_statement("pcmTempo", pcm, 0, length, tempo, nWin, search, positionsIn, positionsOut, format, out, capacity);
}

long long speechPlayer_signalTempo(const void* x, int inFormat, long long length, double tempo, int nWin, int search, const long long* positionsIn,
                                   long long* positionsOut, int format, void* out, long long capacity)
{
    begin_call();
    return tempo_statement("signalTempo", x, inFormat, length, tempo, nWin, search, positionsIn, positionsOut, format, out, capacity);
}

// A row of either tempo export carries its output length and its frames by its own tempo (TempoRow); the export counts frames (the
// positions) or outputs (the render)
static_assert(sizeof(TempoRow) % 8 == 0, "rows are arrays of 8-byte words");
constexpr ExportNouns kFrameNouns{"largest frame count", "frames", nullptr};

// The positions of chosen rows, one workgroup per row, longest first (klatt_tempo.h).  The host path is the other exports': it reads the pool,
// so it is ordered as speechPlayer_batch_exportPcm is (ExportStage, ofPcm).  The staging block: rows | the order.  Nothing is kept on the batch.
static long long tempo_positions_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances,
                                        long long nUtterances, const double* tempo, int nWin, int search, long long* devicePositions, long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (rowStride < 0) { set_error("%s: rowStride %lld", what, rowStride); return -1; }
        TempoPlan P;
        std::string why;
        if (!tempo_plan(P, nWin, search, true, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<TempoRow> rows;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                if (!tempo_of_row(tempo, i, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
                const long long L = in.len(u), Lout = tempo_out_length(L, tempo[i]), K = tempo_frames(Lout, P.Hs);
                rows.push_back(TempoRow{in.at(u), L, Lout, 0, tile_row_first(i, rowStride, before), K, tempo[i]});
                return K;
            }, in.sig)) return -1;
        const long long elements = export_elements(what, kFrameNouns, s, rowStride, 1);
        if (elements <= 0) return elements;
        if (!in.sig && export_synthesised(b, what)) return -1;
        if (export_output(b, what, devicePositions, elements, sizeof(long long)) || signal_memory(in, what, devicePositions, (size_t)elements * sizeof(long long))) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        std::vector<long long> order((size_t)s.n);
        for (long long i = 0; i < s.n; ++i) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](long long a, long long c) { return rows[(size_t)a].frames > rows[(size_t)c].frames; });
        StageBlock block;
        const int rowsAt = block.add(rows), orderAt = block.add(order);
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        TempoSearchArgs A;
        A.in = in.data; A.rows = stage.device<TempoRow>(rowsAt); A.order = stage.device<long long>(orderAt);
        A.nRows = s.n; A.rowStride = rowStride; A.nWin = P.nWin; A.search = P.search; A.pos = devicePositions;
        const unsigned grid = (unsigned)std::min<long long>(s.n, 64ll * b->cus);
        hipLaunchKernelGGL(in.format() ? klatt_tempo_search<float> : klatt_tempo_search<int16_t>, dim3(grid), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportTempoPositions(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const double* tempo, int nWin,
                                                  int search, long long* devicePositions, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportTempoPositions")) return -1;
    return tempo_positions_export("exportTempoPositions", batch, false, nullptr, utterances, nUtterances, tempo, nWin, search, devicePositions, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportTempoPositionsOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
                                                    const double* tempo, int nWin, int search, long long* devicePositions, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportTempoPositionsOf")) return -1;
    return tempo_positions_export("exportTempoPositionsOf", batch, true, signal, rows, nRows, tempo, nWin, search, devicePositions, rowStride, stream);
}

// The chosen rows rendered from positions in device memory, tile-wise (klatt_tempo.h).  The host path is the tile-wise exports'; the positions
// are a device tensor [row][frame] of int64, checked as lpc_residual_export checks its coefficients.  The staging block: rows | tile starts and
// chunk rows (packed) | the window.  Nothing is kept on the batch.
static long long tempo_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances,
                              long long nUtterances, const double* tempo, int nWin, const long long* devicePositions, long long posStride, void* deviceOut, int format,
                              long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        TempoPlan P;
        std::string why;
        if (!tempo_plan(P, nWin, 0, false, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        if (posStride < 0) { set_error("%s: posStride %lld", what, posStride); return -1; }
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        std::vector<TempoRow> rows;
        long long framesBefore = 0, mostFrames = 0;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                if (!tempo_of_row(tempo, i, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
                const long long L = in.len(u), Lout = tempo_out_length(L, tempo[i]), K = tempo_frames(Lout, P.Hs);
                rows.push_back(TempoRow{in.at(u), L, Lout, tile_row_first(i, rowStride, before), tile_row_first(i, posStride, framesBefore), K, tempo[i]});      // (the extent below refuses a stride that wraps)
                framesBefore += K; mostFrames = std::max(mostFrames, K);
                return Lout;
            }, in.sig)) return -1;
        if (posStride > 0 && posStride < mostFrames) { set_error("%s: posStride %lld is below the largest frame count (%lld)", what, posStride, mostFrames); return -1; }
        if (posStride > 0 && mostFrames > 0 && s.n > kExportLimit / posStride) {
            set_error("%s: %lld rows of posStride %lld frames (at most 2^50 elements)", what, s.n, posStride); return -1;
        }
        const long long posFrames = posStride > 0 ? (mostFrames > 0 ? s.n * posStride : 0) : framesBefore;
        if (posFrames > kExportLimit) { set_error("%s: %lld frames of positions (at most 2^50 elements)", what, posFrames); return -1; }
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        const size_t elSize = format ? sizeof(float) : sizeof(int16_t);
        const size_t outBytes = (size_t)elements * elSize, posBytes = (size_t)posFrames * sizeof(long long);
        if (posBytes) {
            if (!devicePositions) { set_error("%s: no positions", what); return -1; }
            const std::string name = std::string(what) + ": positions";
            if (!device_range(devicePositions, posBytes, b->device, sizeof(long long), name.c_str())) return -1;
            const uintptr_t c = reinterpret_cast<uintptr_t>(devicePositions), o = reinterpret_cast<uintptr_t>(deviceOut);
            if (c < o + outBytes && o < c + posBytes) {
                set_error("%s: the output (%zu bytes from %p) overlaps the positions (%zu bytes from %p)", what, outBytes, deviceOut, posBytes, (const void*)devicePositions); return -1;
            }
        }
        hipStream_t st = static_cast<hipStream_t>(stream);
        std::vector<long long> words;
        const TileTable tiles = tile_row_table(s.counts.data(), s.n, kTempoTile, rowStride, kTimelineChunkLog2, words);
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), windowAt = block.add(P.window);
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        TempoArgs A;
        A.in = in.data; A.rows = stage.device<TempoRow>(rowsAt);
        A.tile = tile_out(stage, wordsAt, tiles, rowStride, deviceOut);
        A.pos = devicePositions; A.window = stage.device<float>(windowAt); A.nWin = P.nWin;
        void (*const kernels[2][2])(TempoArgs) = {{klatt_tempo_render<false, int16_t>, klatt_tempo_render<true, int16_t>}, {klatt_tempo_render<false, float>, klatt_tempo_render<true, float>}};
        if (launch_tiles(stage, kernels, in.format(), format, 8, A)) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportTempo(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const double* tempo, int nWin,
                                         const long long* devicePositions, long long posStride, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportTempo")) return -1;
    return tempo_export("exportTempo", batch, false, nullptr, utterances, nUtterances, tempo, nWin, devicePositions, posStride, deviceOut, format, rowStride, stream);
}

// The same of chosen rows of a caller's signal: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportTempoOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, const double* tempo,
                                           int nWin, const long long* devicePositions, long long posStride, void* deviceOut, int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportTempoOf")) return -1;
    return tempo_export("exportTempoOf", batch, true, signal, rows, nRows, tempo, nWin, devicePositions, posStride, deviceOut, format, rowStride, stream);
}

// ---- the PCM mixed with noise and other utterances (klatt_mix.h) ----------------------------------------------------------------------------
static_assert(sizeof(speechPlayer_mixTerm_t) == sizeof(MixTermIn) && offsetof(speechPlayer_mixTerm_t, kind) == offsetof(MixTermIn, kind) &&
              offsetof(speechPlayer_mixTerm_t, levelKind) == offsetof(MixTermIn, levelKind) && offsetof(speechPlayer_mixTerm_t, source) == offsetof(MixTermIn, source) &&
              offsetof(speechPlayer_mixTerm_t, offset) == offsetof(MixTermIn, offset) && offsetof(speechPlayer_mixTerm_t, level) == offsetof(MixTermIn, level) &&
              offsetof(speechPlayer_mixTerm_t, loop) == offsetof(MixTermIn, loop), "klatt_mix.h restates speechPlayer_mixTerm_t");

// Host only, touches no device: the definition of klatt_mix.h through the functions the kernels are compiled from.
// ofSignal (speechPlayer_signalMix): x is int16 or float32 (inFormat); a kind-1 term may name a float32 source, a row of the signal,
// whose power is signal_power's; a float32 source is held to a clip's length only where a kind-0 term names it.
static long long mix_statement(const char* what, bool ofSignal, const void* pcm, int inFormat, long long length, float speechGain, const speechPlayer_mixSource_t* sources,
                               long long nSources, const speechPlayer_mixTerm_t* terms, long long nTerms, float* gains, int format, void* out, long long capacity)
{
    if (ofSignal && signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kMixMaxLength || (length > 0 && !pcm)) { set_error("%s: length %lld (0 .. 2^33, with its samples)", what, length); return -1; }
    if (format != 0 && format != 1) { set_error("%s: format %d (0 int16, 1 float32)", what, format); return -1; }
    if (nSources < 0 || (nSources > 0 && !sources)) { set_error("%s: %lld sources", what, nSources); return -1; }
    if (nTerms < 0 || nTerms > kMixMaxTerms || (nTerms > 0 && !terms)) { set_error("%s: %lld terms (0 .. %d, with their descriptors)", what, nTerms, kMixMaxTerms); return -1; }
    try {
        std::string why;
        if (!mix_check_speech_gain(speechGain, 0, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
        std::vector<MixSource> src((size_t)nSources);
        std::vector<char> powered((size_t)nSources, 0);      // bit `kind`: a float32 source may be named as a clip and as a row, and the two powers differ
        for (long long k = 0; k < nSources; ++k) {
            const speechPlayer_mixSource_t& q = sources[k];
            if (q.format != 0 && q.format != 1) { set_error("%s: source %lld has format %d (0 int16, 1 float32)", what, k, q.format); return -1; }
            // (a float32 source of a signal's mix may be a row: a clip's length is asked of it where a kind-0 term names it)
            if (q.length < 0 || (q.format == 1 && !ofSignal ? q.length < 1 || q.length >= (1ll << 31) : q.length > kMixMaxLength) || (q.length > 0 && !q.data)) {
                set_error("%s: source %lld has %lld samples (a clip 1 .. 2^31 - 1, an utterance 0 .. 2^33, with its samples)", what, k, q.length); return -1;
            }
            if (q.format == 1) {
                const long long bad = mix_bad_value(static_cast<const float*>(q.data), q.length);
                if (bad >= 0) { set_error("%s: sample %lld of clip %lld is %g (finite, at most 2^16 in magnitude)", what, bad, k, (double)static_cast<const float*>(q.data)[bad]); return -1; }
            }
            src[(size_t)k] = MixSource{q.data, q.length, q.format, 0.0};
        }
        const MixTermIn* in = reinterpret_cast<const MixTermIn*>(terms);
        std::vector<MixTermHost> host((size_t)nTerms);
        struct PowerOf { double of[2]; };
        std::vector<PowerOf> powers((size_t)nSources, PowerOf{{0.0, 0.0}});
        double Ps = 0.0;
        bool havePs = false;
        for (long long j = 0; j < nTerms; ++j) {
            const MixTermIn& t = in[j];
            // (one list of sources for both kinds: a clip is a float32 source, an utterance an int16 one)
            if (!mix_check_term(t, 0, j, t.kind == 0 ? nSources : -1, t.kind == 1 ? nSources : 0, [&](int, long long k) { return src[(size_t)k].length; }, why, ofSignal)) {
                set_error("%s: %s", what, why.c_str()); return -1;
            }
            MixSource& q = src[(size_t)t.source];
            if (ofSignal && t.kind == 0 && q.isFloat && (q.length < 1 || q.length >= (1ll << 31))) {
                set_error("%s: row 0, term %lld: clip %lld has %lld samples (1 .. 2^31 - 1)", what, j, t.source, q.length); return -1;
            }
            if (ofSignal ? (t.kind == 0 && !q.isFloat) : q.isFloat != (t.kind == 0)) { set_error("%s: row 0, term %lld: kind %d names source %lld, which is %s", what, j, t.kind, t.source, q.isFloat ? "float32 (a clip)" : "int16 (an utterance)"); return -1; }
            float g = (float)t.level;
            if (t.levelKind == 0) {
                if (!havePs) { Ps = signal_power(pcm, inFormat, length); havePs = true; }      // (of values yet to be checked: it steers nothing)
                double (&known)[2] = powers[(size_t)t.source].of;
                if (!(powered[(size_t)t.source] & (1 << t.kind))) {
                    known[t.kind] = t.kind == 0 ? mix_clip_power(static_cast<const float*>(q.data), q.length) : signal_power(q.data, q.isFloat, q.length);
                    powered[(size_t)t.source] |= (char)(1 << t.kind);
                }
                g = mix_gain(Ps, known[t.kind], mix_ratio(t.level));
            }
            host[(size_t)j] = MixTermHost{(int)t.source, t.offset, t.loop, g};
        }
        if (capacity < length && out) { set_error("%s: the output takes %lld elements, capacity is %lld", what, length, capacity); return -1; }
        if (ofSignal && signal_host_values(what, pcm, inFormat, length)) return -1;
        for (long long j = 0; gains && j < nTerms; ++j) gains[j] = host[(size_t)j].gain;
        if (!out) return length;
        return inFormat ? mix_host(static_cast<const float*>(pcm), length, speechGain, src.data(), host.data(), nTerms, format, out)
                        : mix_host(static_cast<const int16_t*>(pcm), length, speechGain, src.data(), host.data(), nTerms, format, out);
    } catch (const std::exception& e) { set_error("%s: %s", what, e.what()); return -1; }
}

long long speechPlayer_pcmMix(const sample* pcm, long long length, float speechGain, const speechPlayer_mixSource_t* sources, long long nSources,
                              const speechPlayer_mixTerm_t* terms, long long nTerms, float* gains, int format, void* out, long long capacity)
{
    begin_call();
    static_assert(sizeof(sample) == sizeof(int16_t), "a sample is an int16");
    return mix_statement("pcmMix", false, pcm, 0, length, speechGain, sources, nSources, terms, nTerms, gains, format, out, capacity);
}

long long speechPlayer_signalMix(const void* x, int inFormat, long long length, float speechGain, const speechPlayer_mixSource_t* sources, long long nSources,
                                 const speechPlayer_mixTerm_t* terms, long long nTerms, float* gains, int format, void* out, long long capacity)
{
    begin_call();
    return mix_statement("signalMix", true, x, inFormat, length, speechGain, sources, nSources, terms, nTerms, gains, format, out, capacity);
}

// Host only: the power of `length` samples of a signal's row (klatt_sigpower.h: the definition), int16 (mix_power of the exact sum) or float32
int speechPlayer_signalPower(const void* x, int inFormat, long long length, double* power)
{
    begin_call();
    const char* what = "signalPower";
    if (signal_host_format(what, inFormat)) return -1;
    if (length < 0 || length > kMixMaxLength || (length > 0 && !x)) { set_error("%s: length %lld (0 .. 2^33, with its samples)", what, length); return -1; }
    if (!power) { set_error("%s: no output", what); return -1; }
    if (signal_host_values(what, x, inFormat, length)) return -1;
    *power = signal_power(x, inFormat, length);
    return 0;
}

// The batch's noise bank: validated and its clips' powers computed on the host, its samples kept in device memory until the next call
// (nNoise = 0 frees it) or the batch's end, whatever is set or synthesised meanwhile.  Replacing it waits (on the host) for the exports
// that read the old one; the copy has completed when the call returns, so every later export finds the new one.
int speechPlayer_batch_setNoiseBank(speechPlayer_batch_t batch, const float* noise, const long long* noiseStart, long long nNoise)
{
    return (int)batch_entry("setNoiseBank", batch, [&](Batch* b) -> long long {
        MixBank B;
        std::string why;
        if (!mix_bank_plan(B, noise, noiseStart, nNoise, why)) { set_error("setNoiseBank: %s", why.c_str()); return -1; }
        HIP_TRY(hipSetDevice(b->device));
        if (b->bankOrder.used) { HIP_TRY(hipEventSynchronize(b->bankOrder.done)); b->bankOrder.used = false; }
        // From here on the old bank is gone whatever happens: a buffer that must grow is freed first, and a copy that fails may have
        // overwritten a part of one that is reused.  A failure below leaves the batch with no bank rather than with stale starts and powers.
        b->hasBank = false;
        b->bank = MixBank();
        if (nNoise == 0) { b->dBank.release(); return 0; }
        const size_t total = (size_t)B.start.back();
        if (b->dBank.reserve(total)) return -1;
        HIP_TRY(hipMemcpy(b->dBank.ptr, noise, total * sizeof(float), hipMemcpyHostToDevice));
        b->bank = std::move(B);
        b->hasBank = true;
        return 0;
    });
}

long long speechPlayer_batch_noiseBank(speechPlayer_batch_t batch, double* power, long long* length, long long capacity)
{
    return batch_entry("noiseBank", batch, [&](Batch* b) -> long long {
        const long long n = b->hasBank ? b->bank.clips() : 0;
        for (long long k = 0; k < n && n <= capacity; ++k) {
            if (power) power[k] = b->bank.power[(size_t)k];
            if (length) length[k] = b->bank.start[(size_t)k + 1] - b->bank.start[(size_t)k];
        }
        return n;
    });
}

// The distinct rows whose power a call needs -- utterances of the pool, rows of a signal --: a slot each, and the power kernel's walk over
// them: klatt_power's tiles of kPowerTile int16 samples, klatt_signal_power's blocks of kSigPowerBlock float32 ones
struct PowerSlots {
    std::vector<long long> slotOfUtt;      // [rows of the input], -1: none yet
    std::vector<PowerJob> jobs;
    std::vector<long long> tileStart{0};
    long long of(const ExportInput& in, long long u)
    {
        if (slotOfUtt.empty()) slotOfUtt.assign((size_t)in.rows(), -1);
        if (slotOfUtt[(size_t)u] >= 0) return slotOfUtt[(size_t)u];
        const long long slot = (long long)jobs.size(), L = in.len(u), unit = in.format() ? kSigPowerBlock : kPowerTile;
        jobs.push_back(PowerJob{in.at(u), L});
        tileStart.push_back(tileStart.back() + (L + unit - 1) / unit);
        slotOfUtt[(size_t)u] = slot;
        return slot;
    }
    long long tiles() const { return tileStart.back(); }
};

static int launch_power(Batch* b, hipStream_t st, const int16_t* data, const PowerSlots& P, const PowerJob* dJobs, const long long* dTileStart, unsigned long long* dSlots)
{
    if (P.tiles() == 0) return 0;
    PowerArgs A;
    A.pool = data; A.jobs = dJobs; A.tileStart = dTileStart; A.nJobs = (long long)P.jobs.size(); A.nTiles = P.tiles(); A.slots = dSlots;
    const unsigned grid = (unsigned)std::min<long long>(A.nTiles, 8ll * b->cus);
    hipLaunchKernelGGL(klatt_power, dim3(grid), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The powers of a signal's slots as one binary64 each (klatt_sigpower.h).  The call's scratch, all in its staging slot: int16 rows take
// zeroed uint64 slots (klatt_power, then klatt_power_doubles), float32 rows one partial per block (klatt_signal_power, then the row pass).
struct SignalPowerScratch {
    int slotsAt = -1, partialsAt = -1, powersAt = -1;
    std::vector<unsigned long long> zeros;
    // The sections that hold contents: before any reserve()
    void add(StageBlock& block, const ExportInput& in, const PowerSlots& P) { if (!in.format()) { zeros.assign(P.jobs.size(), 0ull); slotsAt = block.add(zeros); } }
    void reserve(StageBlock& block, const ExportInput& in, const PowerSlots& P)
    {
        powersAt = block.reserve(P.jobs.size() * sizeof(double));
        if (in.format()) partialsAt = block.reserve((size_t)P.tiles() * sizeof(double));
    }
};
// More block partials than a call's scratch carries
static int signal_power_cap(const char* what, const ExportInput& in, const PowerSlots& P)
{
    if (!in.sig || !in.format() || P.tiles() <= kSigPowerMaxBlocks) return 0;
    set_error("%s: the rows to be powered take %lld blocks of %d samples (at most 2^24 in one call)", what, P.tiles(), kSigPowerBlock);
    return -1;
}
static int launch_signal_power(const ExportStage& stage, const ExportInput& in, const PowerSlots& P, const SignalPowerScratch& S, int jobsAt, int tilesAt, double*& dPowers)
{
    Batch* b = stage.b;
    const long long n = (long long)P.jobs.size();
    dPowers = const_cast<double*>(stage.device<double>(S.powersAt));      // (the slot is this call's until its event)
    if (n == 0) return 0;
    const PowerJob* dJobs = stage.device<PowerJob>(jobsAt);
    const long long* dTiles = stage.device<long long>(tilesAt);
    if (!in.format()) {
        unsigned long long* dSlots = const_cast<unsigned long long*>(stage.device<unsigned long long>(S.slotsAt));
        if (launch_power(b, stage.st, static_cast<const int16_t*>(in.data), P, dJobs, dTiles, dSlots)) return -1;
        const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 8ll * b->cus);
        hipLaunchKernelGGL(klatt_power_doubles, dim3(grid), dim3(256), 0, stage.st, dSlots, dJobs, n, dPowers);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    double* dPartials = const_cast<double*>(stage.device<double>(S.partialsAt));
    if (P.tiles() > 0) {
        SigPowerArgs A;
        A.data = static_cast<const float*>(in.data); A.jobs = dJobs; A.blockStart = dTiles; A.nJobs = n; A.nBlocks = P.tiles(); A.partials = dPartials;
        const unsigned grid = (unsigned)std::min<long long>(A.nBlocks, 16ll * b->cus);
        hipLaunchKernelGGL(klatt_signal_power, dim3(grid), dim3(256), 0, stage.st, A);
        HIP_TRY(hipGetLastError());
    }
    const unsigned grid = (unsigned)std::min<long long>((n + 3) / 4, 16ll * b->cus);
    hipLaunchKernelGGL(klatt_signal_power_rows, dim3(grid), dim3(256), 0, stage.st, dPartials, dTiles, dJobs, n, dPowers);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The chosen utterances' S_u = sum s(n)^2, one uint64 per row (klatt_mix.h: klatt_power into the zeroed slots of the call's staging block,
// then the deal-out to the rows).  It reads the pool, so it is ordered as speechPlayer_batch_exportPcm is (ExportStage, ofPcm).
// ofSignal and `signal` as spectrogram_export's: the chosen rows' powers P, one binary64 per row (klatt_sigpower.h), by the same deal-out.
static long long power_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances,
                              void* deviceOut, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        ExportSelection s;
        PowerSlots P;
        std::vector<long long> slotOf;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long, long long u, long long) -> long long {
                slotOf.push_back(P.of(in, u));
                return 1;
            }, in.sig)) return -1;
        if (s.n == 0) return 0;
        if (signal_power_cap(what, in, P)) return -1;
        if (!in.sig && export_synthesised(b, what)) return -1;
        if (export_output(b, what, deviceOut, s.n, sizeof(unsigned long long)) || signal_memory(in, what, deviceOut, (size_t)s.n * sizeof(unsigned long long))) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);
        const std::vector<unsigned long long> zeros(in.sig ? 0 : P.jobs.size(), 0ull);
        SignalPowerScratch S;
        StageBlock block;
        const int jobsAt = block.add(P.jobs), tilesAt = block.add(P.tileStart), slotOfAt = block.add(slotOf), slotsAt = block.add(zeros);
        if (in.sig) { S.add(block, in, P); S.reserve(block, in, P); }
        ExportStage stage(b, st, block, nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        const unsigned long long* dealt;      // eight bytes per slot: S_u of the pool, P of a signal
        if (in.sig) {
            double* dPowers;
            if (launch_signal_power(stage, in, P, S, jobsAt, tilesAt, dPowers)) return -1;
            dealt = reinterpret_cast<const unsigned long long*>(dPowers);
        } else {
            unsigned long long* dSlots = const_cast<unsigned long long*>(stage.device<unsigned long long>(slotsAt));      // (the slot is this call's until its event)
            if (launch_power(b, st, b->dPcm.ptr, P, stage.device<PowerJob>(jobsAt), stage.device<long long>(tilesAt), dSlots)) return -1;
            dealt = dSlots;
        }
        const unsigned grid = (unsigned)std::min<long long>((s.n + 255) / 256, 8ll * b->cus);
        hipLaunchKernelGGL(klatt_power_deal, dim3(grid), dim3(256), 0, st, dealt, stage.device<long long>(slotOfAt), s.n, static_cast<unsigned long long*>(deviceOut));
        HIP_TRY(hipGetLastError());
        if (stage.finish()) return -1;
        return s.n;
    });
}

long long speechPlayer_batch_exportPower(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, void* deviceOut, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportPower")) return -1;
    return power_export("exportPower", batch, false, nullptr, utterances, nUtterances, deviceOut, stream);
}

// The same of chosen rows of a caller's signal, as binary64 powers: it reads no pool and needs no synthesis (ExportStage, ofSignal).
long long speechPlayer_batch_exportPowerOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows, void* deviceOut,
                                           void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportPowerOf")) return -1;
    return power_export("exportPowerOf", batch, true, signal, rows, nRows, deviceOut, stream);
}

// The chosen utterances' PCM, row i mixed with its terms terms[termStart[i] .. termStart[i+1]) (klatt_mix.h).  It reads the pool, so it is
// ordered as speechPlayer_batch_exportPcm is (ExportStage, ofPcm), tile-wise; a call that names a clip also takes its place in the bank's order.  The
// staging block: rows | tile starts and chunk rows (packed) | the terms as the kernel reads them | their level jobs | the power slots'
// utterances, tiles and zeros | the gains (reserved: nothing is uploaded).  The slots and the gains are the call's device scratch: they
// live in its staging slot.
// ofSignal and `signal` as spectrogram_export's: the rows and the kind-1 sources are rows of the signal, the powers are klatt_sigpower.h's
// (SignalPowerScratch: behind the gains, reserved as they are), and a call that names a clip still follows the bank's order.
static long long mixed_export(const char* what, speechPlayer_batch_t batch, bool ofSignal, const speechPlayer_signal_t* signal, const long long* utterances, long long nUtterances,
                              const speechPlayer_mixTerm_t* terms, const long long* termStart, const float* speechGain, void* deviceGains, void* deviceOut, int format,
                              long long rowStride, void* stream)
{
    return batch_entry(what, batch, [&](Batch* b) -> long long {
        if (tile_request(what, format, rowStride)) return -1;
        SignalPlan sig;
        ExportInput in{b};
        if (export_input(b, what, ofSignal, signal, sig, in)) return -1;
        const MixTermIn* tin = reinterpret_cast<const MixTermIn*>(terms);
        std::string why;
        ExportSelection s;
        PowerSlots P;
        std::vector<MixRow> rows;
        std::vector<MixTermDev> dev;
        std::vector<MixGainJob> jobs;
        bool readsBank = false;
        double lastDb = 0.0, lastRatio = 1.0;      // pow(10.0, 0.0) is 1
        const long long nClips = b->hasBank ? b->bank.clips() : -1;
        if (export_selection(b, what, utterances, nUtterances, false, s, [&](long long i, long long u, long long before) -> long long {
                if (!mix_check_row(termStart, i, terms, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
                const float sg = speechGain ? speechGain[i] : 1.0f;
                if (!mix_check_speech_gain(sg, i, why)) { set_error("%s: %s", what, why.c_str()); return -1; }
                const long long L = in.len(u), a = termStart[i], nT = termStart[i + 1] - a;
                for (long long j = 0; j < nT; ++j) {
                    const MixTermIn& t = tin[a + j];
                    if (!mix_check_term(t, i, j, nClips, in.rows(), [&](int kind, long long k) {
                            return kind == 0 ? b->bank.start[(size_t)k + 1] - b->bank.start[(size_t)k] : in.len(k);
                        }, why, in.sig != nullptr)) { set_error("%s: %s", what, why.c_str()); return -1; }
                    MixTermDev d;
                    if (t.kind == 0) { d.at = b->bank.start[(size_t)t.source]; d.len = b->bank.start[(size_t)t.source + 1] - d.at; readsBank = true; }
                    else { d.at = in.at(t.source); d.len = in.len(t.source); }
                    d.offset = t.offset; d.flags = (t.kind == 0 ? kMixClip : 0) | (t.loop ? kMixLoop : 0); d.pad = 0;
                    dev.push_back(d);
                    MixGainJob job{1.0, 0.0, 0, -1, (float)t.level, 1};
                    if (t.levelKind == 0) {
                        if (t.level != lastDb) { lastDb = t.level; lastRatio = mix_ratio(t.level); }      // (a batch repeats few levels: one pow each)
                        job.linear = 0; job.gain = 0.0f; job.ratio = lastRatio;
                        job.rowSlot = P.of(in, u);
                        if (t.kind == 0) job.pv = b->bank.power[(size_t)t.source]; else job.srcSlot = P.of(in, t.source);
                    }
                    jobs.push_back(job);
                }
                rows.push_back(MixRow{in.at(u), L, tile_row_first(i, rowStride, before), a, (int)nT, sg});
                return L;
            }, in.sig)) return -1;
        if (signal_power_cap(what, in, P)) return -1;
        const long long elements = tile_elements(b, what, s, rowStride, format, deviceOut, &in);
        if (elements <= 0) return elements;
        const long long nTerms = (long long)dev.size();
        if (deviceGains && nTerms > 0 && !device_range(deviceGains, (size_t)nTerms * sizeof(float), b->device, sizeof(float), what)) return -1;
        if (deviceGains && nTerms > 0 && signal_memory(in, what, deviceGains, (size_t)nTerms * sizeof(float))) return -1;
        hipStream_t st = static_cast<hipStream_t>(stream);

        std::vector<long long> words;
        const TileTable tiles = tile_row_table(s.counts.data(), s.n, kMixTile, rowStride, kTimelineChunkLog2, words);
        const std::vector<unsigned long long> zeros(in.sig ? 0 : P.jobs.size(), 0ull);
        SignalPowerScratch S;
        StageBlock block;
        const int rowsAt = block.add(rows), wordsAt = block.add(words), termsAt = block.add(dev), jobsAt = block.add(jobs), slotJobsAt = block.add(P.jobs),
                  tilesAt = block.add(P.tileStart), slotsAt = block.add(zeros);
        if (in.sig) S.add(block, in, P);
        const int gainsAt = block.reserve((size_t)nTerms * sizeof(float));      // (klatt_mix_gains fills the gains)
        if (in.sig) S.reserve(block, in, P);
        ExportStage stage(b, st, block, readsBank ? &b->bankOrder : nullptr, !in.sig, in.sig != nullptr);
        if (stage.begin()) return -1;
        float* dGains = const_cast<float*>(stage.device<float>(gainsAt));
        const unsigned gainGrid = (unsigned)std::min<long long>((nTerms + 255) / 256, 8ll * b->cus);
        if (in.sig) {
            double* dPowers;
            if (launch_signal_power(stage, in, P, S, slotJobsAt, tilesAt, dPowers)) return -1;
            if (nTerms > 0) {
                hipLaunchKernelGGL(klatt_mix_gains_of, dim3(gainGrid), dim3(256), 0, st, stage.device<MixGainJob>(jobsAt), nTerms, dPowers, dGains, static_cast<float*>(deviceGains));
                HIP_TRY(hipGetLastError());
            }
        } else {
            unsigned long long* dSlots = const_cast<unsigned long long*>(stage.device<unsigned long long>(slotsAt));      // (the slot is this call's until its event)
            if (launch_power(b, st, b->dPcm.ptr, P, stage.device<PowerJob>(slotJobsAt), stage.device<long long>(tilesAt), dSlots)) return -1;
            if (nTerms > 0) {
                hipLaunchKernelGGL(klatt_mix_gains, dim3(gainGrid), dim3(256), 0, st, stage.device<MixGainJob>(jobsAt), nTerms, dSlots, stage.device<PowerJob>(slotJobsAt),
                                   dGains, static_cast<float*>(deviceGains));
                HIP_TRY(hipGetLastError());
            }
        }
        MixArgs A;
        A.pool = in.data; A.bank = b->dBank.ptr; A.rows = stage.device<MixRow>(rowsAt);
        A.tile = tile_out(stage, wordsAt, tiles, rowStride, deviceOut);
        A.terms = stage.device<MixTermDev>(termsAt); A.gains = dGains;
        void (*const kernels[2][2])(MixArgs) = {{klatt_mix<false, int16_t>, klatt_mix<true, int16_t>}, {klatt_mix<false, float>, klatt_mix<true, float>}};
        if (launch_tiles(stage, kernels, in.format(), format, 8, A)) return -1;
        return elements;
    });
}

long long speechPlayer_batch_exportMixed(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const speechPlayer_mixTerm_t* terms,
                                         const long long* termStart, const float* speechGain, void* deviceGains, void* deviceOut, int format,
                                         long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportMixed")) return -1;
    return mixed_export("exportMixed", batch, false, nullptr, utterances, nUtterances, terms, termStart, speechGain, deviceGains, deviceOut, format, rowStride, stream);
}

// The same onto chosen rows of a caller's signal, termStart and speechGain per output row: it reads no pool and needs no synthesis
// (ExportStage, ofSignal).
long long speechPlayer_batch_exportMixedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
                                           const speechPlayer_mixTerm_t* terms, const long long* termStart, const float* speechGain, void* deviceGains, void* deviceOut,
                                           int format, long long rowStride, void* stream)
{
    if (refuse_timing_only("speechPlayer_batch_exportMixedOf")) return -1;
    return mixed_export("exportMixedOf", batch, true, signal, rows, nRows, terms, termStart, speechGain, deviceGains, deviceOut, format, rowStride, stream);
}

}  // extern "C"
