// check_stage_frames.cpp -- a host model of the signal stages on the step grid (csrc/klatt_stage_frames.h: LPC and the pitch) in a program of
// its own, built by tests/test_stage_frames_host.py with AddressSanitizer + UBSan.  It drives klatt_stage.h's bookkeeping (stage_row_plan,
// stage_lpc_frames / stage_pitch_frames, stage_frames_emitted, stage_sample, stage_history_from_chunk, stage_row_advance) over random
// chunkings, ends and resets, as the kernels' entry points do: every emitted step's frame, read through the virtual row, must equal the frame
// of the concatenated stream, and lpc_frame_host / pitch_frame_host on it must equal lpc_host / pitch_host of the whole stream bit for bit.
// Every chunk lives in an allocation of exactly its size, so a read outside it is an error the sanitizer reports.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../nvspeechplayer_amd/csrc/klatt_stage_frames.h"

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

// A chunk: int16 or float32 samples in an allocation of exactly its size -- a tone of period 37.3 with noise, and runs of exact zeros --
// and the same appended to the statements' float32 input
struct Chunk {
    bool f32 = false;
    std::vector<int16_t> s;
    std::vector<float> x;
    long long len() const { return (long long)(f32 ? x.size() : s.size()); }
};
static Chunk make_chunk(long long c, std::vector<float>& whole)
{
    Chunk k;
    k.f32 = rnd() & 1;
    for (long long i = 0; i < c; ++i) {
        const long long n = (long long)whole.size();
        const bool silent = (n / 900) % 3 == 2;
        const double v = silent ? 0.0 : 0.6 * sin(6.283185307179586 * (double)n / 37.3) + 0.05 * ((double)(long long)(rnd() % 2001) / 1000.0 - 1.0);
        if (k.f32) { k.x.push_back((float)v); whole.push_back(k.x.back()); }
        else { k.s.push_back((int16_t)(int)(v * 20000.0)); whole.push_back(tile_x((int)k.s.back())); }
    }
    return k;
}

static bool same_bits(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

struct RowModel {
    long long N = 0, M = 0;
    std::vector<float> hist;
};

// The next history: the last H of [history | chunk], zeros behind an end
template <typename In>
static void next_history(RowModel& r, const In* chunk, long long c, bool ended)
{
    const int H = (int)r.hist.size();
    std::vector<float> next((size_t)H, 0.0f);
    for (int j = 0; j < H && !ended; ++j) {
        long long at;
        next[(size_t)j] = stage_history_from_chunk(j, H, c, at) ? tile_x(chunk[at]) : r.hist[(size_t)at];
    }
    r.hist = next;
}

// What a kind does with a frame of n samples: o[nCols] from x[n]
struct Kind {
    StageGeometry g;
    int n = 0, nCols = 0;
    LpcPlan lpc;
    PitchPlan pitch;
    void fields(const float* x, double* o) const
    {
        if (g.kind == kStageLpc) {
            std::vector<float> xw((size_t)n);
            for (int i = 0; i < n; ++i) xw[(size_t)i] = spec_windowed(x[i], lpc.window[(size_t)i]);
            lpc_frame_host(xw.data(), lpc, o);
        } else {
            std::vector<double> m((size_t)pitch.lagMax + 2);
            pitch_frame_host(x, pitch, m.data(), o);
        }
    }
};

// A push: the steps the plan says, each frame through the virtual row -- the kernels' first sample phase + (M + e) hop - floor(n / 2)
template <typename In>
static void push(const Kind& K, RowModel& r, const In* chunk, long long c, bool ended, const std::vector<float>& whole, long long base, std::vector<double>& out)
{
    const StageFrames& f = K.g.frames;
    const int H = stage_frame_history(f);
    long long n;
    CHECK(stage_has_frames(K.g.kind) && stage_keeps_history(K.g.kind) && stage_row_plan(K.g, H, r.N, r.M, c, ended, n) && n >= 0);
    CHECK(n == stage_frames_emitted(f, r.N + c, ended) - r.M);
    CHECK(H == K.n - 1 && (int)r.hist.size() == H && f.before == K.n / 2 && f.before + f.after + 1 == K.n);
    std::vector<float> frame((size_t)K.n);
    for (long long e = 0; e < n; ++e) {
        const long long t0 = f.phase + (r.M + e) * f.hop - K.n / 2;
        CHECK(t0 == stage_frame_centre(f, r.M + e) - f.before);
        CHECK(t0 >= r.N - H);                                                       // the lemma
        CHECK(stage_frame_centre(f, r.M + e) + f.after < r.N + c || ended);         // a frame past the stream's samples is an ended row's alone
        for (int i = 0; i < K.n; ++i) {
            frame[(size_t)i] = stage_sample(r.hist.data(), chunk, t0 + i, r.N, H, c);
            // ... and it is the concatenated stream's sample: `whole` holds the row's samples since its start from `base` on
            const float want = tile_sample(whole.data() + base, t0 + i, r.N + c);
            CHECK(same_bits(&frame[(size_t)i], &want, sizeof(float)));
        }
        out.resize(out.size() + (size_t)K.nCols);
        K.fields(frame.data(), out.data() + out.size() - (size_t)K.nCols);
    }
    next_history(r, chunk, c, ended);
    stage_row_advance(r.N, r.M, c, ended, n);
}

// A stream of chunks onto one row; `resetAt` >= 0: the row is reset before that chunk, and the statement is of what follows
static void stream(const Kind& K, RowModel& r, const std::vector<long long>& lens, int resetAt = -1)
{
    std::vector<float> whole;
    std::vector<double> got;
    long long base = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
        if ((int)i == resetAt) {      // klatt_stage_clear_rows and the host's N = M = 0
            std::fill(r.hist.begin(), r.hist.end(), 0.0f);
            r.N = r.M = 0;
            base = (long long)whole.size();
            got.clear();
        }
        const Chunk k = make_chunk(lens[i], whole);
        const bool ended = i + 1 == lens.size();
        if (k.f32) push(K, r, k.x.data(), k.len(), ended, whole, base, got); else push(K, r, k.s.data(), k.len(), ended, whole, base, got);
        if (!ended) CHECK((long long)got.size() == stage_frames_emitted(K.g.frames, r.N, false) * K.nCols && r.M * K.nCols == (long long)got.size());
    }
    CHECK(r.N == 0 && r.M == 0);
    const long long L = (long long)whole.size() - base, hop = K.g.frames.hop, phase = K.g.frames.phase;
    const long long steps = L > phase ? (L - phase + hop - 1) / hop : 0;
    std::vector<double> want((size_t)(steps * K.nCols) + 1);
    const long long n = K.g.kind == kStageLpc ? lpc_host(whole.data() + base, L, K.lpc, hop, phase, want.data()) : pitch_host(whole.data() + base, L, K.pitch, hop, phase, want.data());
    CHECK(n == (long long)got.size());
    CHECK(same_bits(got.data(), want.data(), (size_t)n * sizeof(double)));
    for (float v : r.hist) CHECK(v == 0.0f);
}

static void check_kind(const Kind& K)
{
    const StageFrames& f = K.g.frames;
    const long long n = K.n, hop = f.hop;
    // the counts against brute force
    for (long long N = 0; N <= 3 * n + hop; ++N) {
        long long open = 0, ended = 0;
        for (long long j = 0; j <= N; ++j) {
            if (f.phase + j * hop + f.after <= N - 1) ++open;
            if (f.phase + j * hop < N) ++ended;
        }
        CHECK(stage_frames_emitted(f, N, false) == open && stage_frames_emitted(f, N, true) == ended);
    }
    RowModel r;
    r.hist.assign((size_t)stage_frame_history(f), 0.0f);
    const long long H = n - 1, pool[8] = {0, 1, H - 1, H, H + 1, hop, hop - 1, 3 * n + 1};
    stream(K, r, {0, 1, H - 1, H, H + 1, hop, 2 * n, 37});
    stream(K, r, {2 * n, hop, H + 1, H, H - 1, 1, 0, 3});
    stream(K, r, {1, 0, n / 2 - 5 > 0 ? n / 2 - 5 : 0, 0});      // below one frame until it ends
    stream(K, r, {n, 5, 0});                                     // an end with an empty last chunk
    stream(K, r, {0});
    stream(K, r, {2800});                                        // past a run of zeros longer than a frame
    stream(K, r, {n, 3, 2, n + hop, 7}, 3);                      // a reset behind two pushes shorter than H: the history mixed old history and chunk
    for (int s = 0; s < 6; ++s) {
        std::vector<long long> lens;
        for (int i = 0; i < 7; ++i) lens.push_back(pool[rnd() % 8]);
        stream(K, r, lens, s % 2 ? (int)(rnd() % 7) : -1);
    }
}

static void check_lpc(int order, int nWin, long long hop, long long phase, int what, bool lag)
{
    Kind K;
    std::string why;
    std::vector<double> lw;
    for (int k = 0; k <= order; ++k) lw.push_back(k == 0 ? 1.0 + 1e-9 : exp(-0.0005 * k * k));
    CHECK(lpc_plan(K.lpc, order, nWin, nullptr, lag ? lw.data() : nullptr, what, why));
    K.g.kind = kStageLpc; K.g.frames = stage_lpc_frames(nWin, hop, phase);
    K.n = nWin; K.nCols = K.lpc.nCols;
    CHECK(K.nCols == lpc_columns(what, order));
    check_kind(K);
}

static void check_pitch(int W, int lagMin, int lagMax, long long hop, long long phase, int what)
{
    Kind K;
    std::string why;
    CHECK(pitch_plan(K.pitch, 16000, W, lagMin, lagMax, 0.15, what, why));
    K.g.kind = kStagePitch; K.g.frames = stage_pitch_frames(W, lagMax, hop, phase);
    K.n = W + lagMax; K.nCols = K.pitch.nCols;
    CHECK(K.nCols == pitch_columns(what, lagMin, lagMax));
    check_kind(K);
}

int main()
{
    check_lpc(4, 33, 8, 0, kLpcAllFields, false);            // an odd window: (before, after) = (16, 16)
    check_lpc(16, 128, 40, 0, kLpcCoeff | kLpcError, true);  // an even one: (64, 63)
    check_lpc(32, 200, 300, 90, kLpcAllFields, false);       // a hop above the frame skips samples
    check_lpc(9, 64, 64, 63, kLpcAutocorr | kLpcStages, false);
    check_pitch(32, 2, 65, 8, 0, kPitchAllFields);           // Nf = 97, odd
    check_pitch(32, 2, 64, 24, 5, kPitchF0 | kPitchVoiced | kPitchPeriod);      // Nf = 96, even: (48, 47)
    check_pitch(64, 20, 100, 300, 170, kPitchAllFields);     // a hop above the frame
    // the refusals of the plan: a negative chunk, a row that would pass 2^44 samples
    StageGeometry g;
    g.kind = kStagePitch; g.frames = stage_pitch_frames(64, 100, 16, 0);
    long long n;
    CHECK(stage_row_plan(g, 163, kResampleMaxLength - 5, 0, 5, false, n) && !stage_row_plan(g, 163, kResampleMaxLength - 5, 0, 6, false, n) &&
          !stage_row_plan(g, 163, 0, 0, -1, false, n));
    printf("ok %lld\n", g_checks);
    return 0;
}
