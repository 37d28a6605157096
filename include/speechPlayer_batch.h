/*
 * speechPlayer_batch.h -- additive batch entry points of the MI355X Klatt engine.
 *
 * The reference has no batch interface: one handle is one stream
 * (reference src/speechPlayer.cpp:19-23) and a caller loops
 * speechPlayer_queueFrame / speechPlayer_synthesize per stream
 * (test_speakIpa.py:24-27, nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:62-81,222-233).
 * A batch replaces N such loops: N frame streams in, N int16 PCM streams out, one
 * utterance per wavefront lane on the GPU.  Every utterance behaves exactly like a
 * fresh handle that had all its frames queued (no purge) and was drained.
 *
 * Plain C: host pointers and sizes only.  All functions return 0 on success and a
 * negative value on failure unless stated; speechPlayer_lastError() describes it.
 *
 * Threads.  DISTINCT batch objects, node objects, signal stages and live handles may be used from distinct threads at the
 * same time, in any mix of calls: each batch has streams, scratch and cached tables of its own, and what the process shares
 * -- the host worker pool the set calls plan on, the registries of stages and live handles -- is locked inside.  ONE batch
 * object (and one node object) is used by one thread at a time; it may be handed from thread to thread -- a set call on a
 * worker thread, the launch and the reads on another, as bench.py's `pipeline` extra does -- with the order kept by the
 * caller (the hand-over must synchronise the two threads: a semaphore, an event, a join).  A signal stage belongs to the
 * batch object it was made on and is used under the same rule, together with it; a stage handle that was freed is refused
 * by whichever thread presents it, and so long as the caller makes no new stage in between it names no other stage.
 * speechPlayer_lastError() and speechPlayer_lastErrorCode() are per calling thread: the code is 0 after that thread's
 * last call succeeded, the message is that of the thread's last failure (empty for a thread that never had one) -- no
 * thread sees another's.  The global option "plan_hash_bits" is read once per set call (and once per planning view):
 * changing it beside a set call in flight changes nothing of that call.
 * tests/test_concurrent_players_host.py and tests/test_gpu_concurrent_players.py hold exactly this.
 */
#ifndef NVSP_AMD_SPEECHPLAYER_BATCH_H
#define NVSP_AMD_SPEECHPLAYER_BATCH_H

#include "speechPlayer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void* speechPlayer_batch_t;

/* Arithmetic modes (speechPlayer_batch_setOption(b, "mode", ...)). */
#define SPEECHPLAYER_MODE_EXACT 0 /* f64, separate rounding of every operation, libm-grade coefficients */
#define SPEECHPLAYER_MODE_FAST 1  /* f64 state, the resonators' multiply-adds fused (within the tolerance, not bit-exact by construction) */

/* Bind a batch engine to HIP device `device` (-1: the current device). NULL on failure. */
speechPlayer_batch_t speechPlayer_batch_create(int sampleRate, int device);
void speechPlayer_batch_destroy(speechPlayer_batch_t batch);

/* Options: "mode" (see above); "sort" (1: pack wavefronts by utterance length, default 1);
 * "layout" (-1: chosen per batch, default; 2: lane-pipelined workgroups for the quiet, nasal-free utterances
 * whatever the batch size; 1: stage-parallel workgroups, four wavefronts per 64 utterances; 0: one wavefront
 * per 64 utterances);
 * "tracks" (1, default: noisy utterances whose parameters are all finite take what they need on fade samples -- resonator
 * coefficients, interpolated gains -- from tracks: evaluated densely by a kernel of its own before the synthesis kernel, one
 * track per distinct fade of the batch, instead of exp/cos, interpolation and a frame state machine inside the sample
 * recurrence; 0: never) and "track_budget_mb" (device memory the tracks of a batch may take, default 4096, which is also the most: the flat stages address the tracks with 32-bit byte offsets; a batch whose
 * tracks do not fit runs without them);
 * "direct" (what runs the noisy, finite utterances that got no tracks -- a batch whose fades share nothing would need 12 bytes of
 * track per output sample: 1, default: the direct stages (every fade sample's coefficients computed in place from per-frame
 * seeds, eight wavefronts per 64 utterances) unless -- in MODE_EXACT -- the utterances are time-aligned copies of few sentences,
 * which the stages with the frame state machine run faster; 2: the direct stages always; 0: never).
 * "quiet_last" (1, default: a launch queues the quiet groups' kernels behind the noisy groups', whose few long workgroups then start first;
 * 0: in front; read by every launch).
 * "dead_terms" (1, default: a wavefront of the tracked group none of whose utterances has voice turbulence, aspiration or a first
 * parallel resonator that contributes -- voiceTurbulenceAmplitude / aspirationAmplitude +0.0 in every frame; pa1 zero with pb1 in
 * [1, 1e6], |pf1| <= 1e6, |fricationAmplitude| and |preFormantGain| <= 1e30 in every frame: all speech of the built-in producer's
 * phoneme table has no turbulence and no pa1 -- runs stage bodies without those terms, which add exactly nothing; 0: every wavefront
 * runs the general bodies.  Same PCM either way.  speechPlayer_batch_kernelInfo reports how many wavefronts of the last launch did, as
 * the stages counted them -- before a batch's first launch: how many will, by the plan and the option as it stands.
 * The same option, by the same rule, drops four more pieces where no utterance of the wavefront has them: the nasal pair N0 / NP from the
 * source stage (caNP zero of either sign in every frame, cbN0 in [1, 1e6], cbNP in [0, 1e6], |cfN0|, |cfNP| <= 1e6, |voiceAmplitude|,
 * |aspirationAmplitude|, |preFormantGain| and the pitches <= 1e30; taken together with the turbulence: m, n and ng alone set caNP); parallel resonator 5, or 5 and
 * 6, from the final stage; parallel resonators 1..4 from the parallel stage (each pa_k zero of either sign with pb_k in [1, 1e6],
 * |pf_k| <= 1e6, |fricationAmplitude| and |preFormantGain| <= 1e30 in every frame: stops, affricates, sh, zh and the flap alone set
 * pa2..pa5).  What is dropped is a finite value times zero; where a zero's sign differs from the general bodies' it stays a zero up to the
 * int16.  kernelInfo: four more counts, of wavefronts whose stage ran without the nasal pair / parallel 5 / parallel 5 and 6 / parallel 1..4.)
 * "direct_lean" (the direct stages' residency: 1 two workgroups per CU, 0 one, -1, default: the engine's choice by mode, size and
 * whether the resident batch's direct group is time-aligned).
 * Read by:
 *   "sort", "track_budget_mb", "direct"   the next set call (any of the speechPlayer_batch_set* entry points): set them before it;
 *                                          changed afterwards they do nothing until the next one.
 *   "mode"                                 every launch (the arithmetic) and the next set call (the routing of "direct" = 1 and
 *                                          whether tracks pay): a launch in the other mode runs the plan as it was made.
 *   "layout"                               the next set call (whether a direct group is formed, whether lonely quiet utterances
 *                                          join the noisy ones) and every launch (which kernel runs each group of the plan as it
 *                                          was made: 0 runs the quiet and the once-tracked groups on the lane kernel, 2 the
 *                                          quiet nasal-free group on the lane-pipelined one; a direct group stays on its stages).
 *   "tracks"                               the next set call (whether tracks are planned) and every launch: 0 runs a planned
 *                                          tracked group on the stages with the frame state machine; 1 after a set call under 0
 *                                          finds no tracks and changes nothing.
 *   "direct_lean", "quiet_last", "dead_terms"   every launch.
 *   "pitch_table_mb", "source_table_mb", "source_lane_lists"   every export that builds the table they bound.
 * No option, whenever it is changed, changes the PCM of MODE_EXACT, the lengths or the index marks; MODE_FAST stays within its
 * tolerance whichever kernel runs (the direct stages advance the coefficients of a fade by recurrences, re-seeded exactly at every
 * fade's first sample: relative error <= 4 F 2^-53 after F fade samples).  The exports of the batch as set read no option but the
 * three of their tables.  tests/test_gpu_player_script.py changes each between a set call and a launch. */
int speechPlayer_batch_setOption(speechPlayer_batch_t batch, const char* name, int value);

/*
 * Describe the batch and make it resident in HBM (host arrays are copied).
 *   frameStart[nUtterances+1]  utterance u owns frames frameStart[u] .. frameStart[u+1]-1
 *   frames[nFrames]            what each speechPlayer_queueFrame call would have been given
 *   minFrameDuration/fadeDuration[nFrames]  in samples, as in speechPlayer_queueFrame
 *   userIndex[nFrames]         may be NULL (all -1)
 *   isNull[nFrames]            may be NULL (none); nonzero = the call passed framePtr==NULL
 *   noiseSeed[nUtterances]     may be NULL (seed = utterance number); selects the utterance's
 *                              noise stream (the reference's rand() is process-global,
 *                              src/speechWaveGenerator.cpp:40; the engine defines one stream per
 *                              utterance instead -- see DESIGN.md "Noise")
 */
int speechPlayer_batch_setUtterances(speechPlayer_batch_t batch, long long nUtterances, const long long* frameStart,
	const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, const unsigned int* noiseSeed);

/*
 * The same batch in COMPACT form: frame lists that utterances SHARE, and frames as 32-byte records the device expands.
 * The reference produces frames lazily, one utterance at a time (ipa.py:336-353), and hands each to speechPlayer_queueFrame as a
 * 376-byte struct (src/frame.cpp:90-101).  A batch of N utterances seldom holds N different frame streams (BASELINE's configurations
 * are 512 streams instanced), and a frame a producer emits is one of a few hundred parameter vectors plus a pitch pair and two
 * durations.  Both entry points describe `nLists` frame lists once and say per utterance which list it speaks (listOf[u]; NULL:
 * utterance u speaks list u, nUtterances == nLists); utterances of one list read the same frames in HBM and differ in their noise
 * seed alone.  Everything else is as in speechPlayer_batch_setUtterances (each utterance a fresh handle with the list's frames queued).
 *   speechPlayer_batch_setUtterancesShared   the lists as full frames (listStart[nLists+1] into frames / durations / ...)
 *   speechPlayer_batch_setRecords            the lists as records: record k stands for the frame whose parameters 1..45 are
 *                                            shapes[records[k].shape] and whose voicePitch / endVoicePitch are the record's own
 *                                            (shape SPEECHPLAYER_RECORD_SILENCE: framePtr == NULL).  32 bytes per frame cross the
 *                                            link, the 376-byte frames are built in HBM (klatt_expand_frames), and the planner
 *                                            recognises equal frames by their shape number -- exactly, nothing is hashed.
 */
#define SPEECHPLAYER_RECORD_SILENCE 0xFFFFFFFFu
typedef struct {
	double voicePitch, endVoicePitch;             /* parameters 0 and 46 of the frame */
	unsigned int shape;                           /* row of the call's shape table, or SPEECHPLAYER_RECORD_SILENCE */
	unsigned int minFrameDuration, fadeDuration;  /* samples, as in speechPlayer_queueFrame */
	int userIndex;                                /* -1: none */
} speechPlayer_frameRecord_t;                     /* 32 bytes */
int speechPlayer_batch_setUtterancesShared(speechPlayer_batch_t batch, long long nLists, const long long* listStart,
	const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, long long nUtterances, const unsigned int* listOf, const unsigned int* noiseSeed);
int speechPlayer_batch_setRecords(speechPlayer_batch_t batch, long long nShapes, const speechPlayer_frame_t* shapes,
	long long nLists, const long long* listStart, const speechPlayer_frameRecord_t* records,
	long long nUtterances, const unsigned int* listOf, const unsigned int* noiseSeed);
/*
 * The batch of speechPlayer_batch_setUtterances with the 47-double frames in DEVICE memory (a tensor a model or tensor ops computed):
 * same lengths, PCM, index marks, speechPlayer_batch_frames readback and plan.  Only the frames' place differs.
 *   deviceFrames[frameStart[nUtterances]]  device memory of the batch's device (hipMalloc'd, e.g. a torch tensor), 8-byte aligned; the
 *                              call copies it device to device into the batch's own buffer: once it returns the caller may free or
 *                              overwrite it.  frameStart, the durations, userIndex, isNull and noiseSeed stay HOST arrays (the host
 *                              plans with them: 16 bytes per frame against 376).
 *   readyStream                a hipStream_t on which the frames are being produced: the engine records an event there and its copy
 *                              waits for it on the device -- the caller's stream is never synchronised from the host.  NULL: the
 *                              caller guarantees the frames are ready (so frames produced on the NULL stream itself must be handed
 *                              over with a stream that waits for it: BatchPlayer.setUtterancesTensor does so).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT, the previous batch left in place: a host pointer (page-locked memory included), memory of
 * another device, managed memory, a pointer the HIP runtime does not know, one not 8-byte aligned, and frames that run past the end of
 * their allocation.  The frames are looked at on the device (klatt_frame_facts: 24 bytes per frame come back); for the track planner
 * one frame per distinct shape is gathered there and downloaded.
 */
int speechPlayer_batch_setUtterancesDevice(speechPlayer_batch_t batch, long long nUtterances, const long long* frameStart,
	const speechPlayer_frame_t* deviceFrames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, const unsigned int* noiseSeed, void* readyStream);
/*
 * The PCM of chosen utterances into CALLER-OWNED device memory, typed and ordered on the caller's stream.
 *   utterances[nUtterances]    host array of utterance numbers, any order, repeats allowed; NULL: every utterance in order
 *                              (nUtterances is then ignored)
 *   deviceOut                  device memory of the batch's device, aligned to the element size (16-byte alignment takes the vector
 *                              stores), holding the return value's number of elements
 *   format                     0 int16; 1 float32 = sample / 32767 (as speechPlayer_batch_readFloat)
 *   rowStride                  > 0: row i (utterance utterances[i]) starts at element i * rowStride, the elements past the utterance's
 *                              end are 0 -- a rowStride below the longest chosen utterance is refused; 0: the utterances back to back
 *                              in the order given
 *   stream                     a hipStream_t of the batch's device (NULL: the null stream)
 * Returns the number of elements written (0 writes nothing and needs no buffer), -1 on error.  Ordering by events, no host waits: the
 * export runs on `stream` after the batch's last synthesis launch (all its streams), and the batch's next launch waits on the device
 * for the export before it overwrites the pool (a set call leaves the pool alone, unless it must grow it: then it waits for the
 * exports on the host before it frees the old one).  On return the work is queued, nothing has been synchronised (with more than sixteen
 * exports of one batch in flight the seventeenth waits for the first).  The batch must have been synthesised since it was set.
 */
long long speechPlayer_batch_exportPcm(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	void* deviceOut, int format, long long rowStride, void* stream);
/*
 * The timeline of a batch and its per-sample parameter tracks: what was spoken when, and the frame the synthesiser used on a given
 * sample -- the reference's getCurrentFrame() (src/frame.cpp:121-126), which a handle's caller can follow between pulls
 * (speechPlayer_getLastIndex) and a batch's caller could not.  For utterance u of a set batch, of length L, and sample t in 0 .. L-1:
 *   track(u, c, t), c in 0 .. 46 (the order of speechPlayer_frame_t): field c of the frame getCurrentFrame() returned for sample t of a
 *       fresh handle that had the utterance's frames queued, the reference's quirks included: sample 0 and every sample on which a request
 *       is dequeued see the frame of the sample before (all zeros at t = 0); a NaN target holds (src/utils.h:20-23) and the hold after such
 *       a fade keeps the value of the fade's last sample; a NULL request fades to the previous request's values with preFormantGain 0 and
 *       the pitch frozen; voicePitch glides by one addition per hold sample (src/frame.cpp:77), and a real frame with minFrameDuration 0
 *       makes it infinite or NaN (src/frame.cpp:98)
 *   SPEECHPLAYER_TRACK_MARK   what speechPlayer_getLastIndex answers after sample t has been generated
 *   SPEECHPLAYER_TRACK_FRAME  the number, within the utterance, of the request most recently dequeued (0 at t = 0)
 * Request k is dequeued on sample S_k = sum_{i<k} (max(M_i, F_i + 1) + 1), F_i = max(fadeDuration_i, 1); S_n = L.  The tracks are a function
 * of the batch as set: they do not depend on the mode, the layout, the planner's choices or on whether the batch has been synthesised.
 */
#define SPEECHPLAYER_TRACK_MARK  47
#define SPEECHPLAYER_TRACK_FRAME 48
/* Host only, touches no device (like speechPlayer_planDirect): firstSample[frameStart[nUtterances]] = S_k of every request,
 * length[nUtterances] = L_u (either may be NULL).  Returns the number of frames, -1 on bad arguments. */
long long speechPlayer_planTimeline(long long nUtterances, const long long* frameStart, const unsigned int* minFrameDuration,
	const unsigned int* fadeDuration, long long* firstSample, long long* length);
/* The same for utterance u of a set batch (any of the set calls, shared lists and records included), with its marks: returns the
 * utterance's number of frames n; fills firstSample[n + 1] and userIndex[n] (each may be NULL) when n <= capacity. */
long long speechPlayer_batch_timeline(speechPlayer_batch_t batch, long long utterance, long long* firstSample, int* userIndex,
	long long capacity);
/* Tracks of chosen utterances into caller-owned device memory on the caller's stream.  Step j of an utterance is sample
 * phase + j * hop; an utterance has ceil((L - phase) / hop) steps (0 when L <= phase).  Element (i, j, q) =
 * track(utterances[i], columns[q], phase + j * hop).
 *   columns[nColumns]   0 .. 48, any order, repeats allowed
 *   format              0 float64 (the value itself), 1 float32 (the value rounded to nearest; marks beyond 2^24 lose bits)
 *   rowStride           > 0: row i starts at element i * rowStride * nColumns, steps past the utterance's end are 0; below the
 *                       largest step count it is refused; 0: the utterances back to back
 * utterances / nUtterances / deviceOut / stream as in speechPlayer_batch_exportPcm (deviceOut aligned to the element size; 16-byte
 * alignment takes the vector stores).  Returns the elements written (0 writes nothing and needs no buffer), -1 on error.
 * Ordering by events, no host waits: the export needs no synthesis launch -- it is valid as soon as the set call has returned (what
 * that call left queued on the device is waited for by an event) and does not wait for a running launch; the NEXT set call, which
 * replaces the frames the export reads, waits for the exports in flight: on the device where the buffers are reused, on the host where
 * one is freed or where pageable frames are copied outside the streams' order.  With more than sixteen exports of one batch in flight
 * the seventeenth waits for the first.  voicePitch (column 0) is carried through a table of 8 bytes per (frame list, step); an export
 * whose table would exceed option "pitch_table_mb" (default 256) proceeds in pieces of utterances, and exports that ask for column 0
 * follow one another on the device.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, a column outside 0 .. 48, nColumns <= 0, hop <= 0, phase < 0, an
 * unknown format, an utterance number outside the batch, a rowStride below the largest step count, an output that is not device memory
 * of the batch's device, misaligned or too small. */
long long speechPlayer_batch_exportTracks(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const int* columns, int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride, void* stream);
/*
 * The glottal source of a batch: what the voice source did on every sample -- the fundamental after vibrato, the glottal phase, whether
 * the glottis is open, and the sample on which every glottal cycle begins (the pitch marks).  The synthesiser computes these from two
 * running sums that it rounds once per sample (FrequencyGenerator, reference src/speechWaveGenerator.cpp:46-60, :72-77) and keeps none
 * of them; re-adding the exported tracks elsewhere gives another phase and, now and then, a pitch mark on another sample.
 * For utterance u of a set batch, of length L, at sample rate sr, let cur(t) be the frame speechPlayer_batch_exportTracks defines for
 * sample t (its quirks included: sample 0 and every dequeue sample see the frame of the sample before, NaN holds, NULL requests, the
 * voicePitch glide).  With V(-1) = P(-1) = 0 and C(-1) = 0, for t = 0 .. L-1, every operation rounded separately in binary64, in this order:
 *   frac(x)  = x - trunc(x)                           (fmod(x, 1) except for the sign of a zero; NaN for a non-finite x)
 *   V(t)     = frac(vibratoSpeed(t) / sr + V(t-1))    (the vibrato phase advances at zero depth too)
 *   vib(t)   = sin(V(t) * 6.283185307179586) * 0.06 * vibratoPitchOffset(t) + 1
 *   hz(t)    = voicePitch(t) * vib(t)
 *   x(t)     = hz(t) / sr + P(t-1)
 *   P(t)     = frac(x(t))
 *   epoch(t) = x(t) is finite and |x(t)| >= 1
 *   C(t)     = C(t-1) + epoch(t)
 * -- what the source stage of every synthesis kernel does with cur(t), by the same device functions on the same operands in the same
 * order, so the exported phase is the phase behind the PCM.  The phases advance on every sample, through silence as well.  The result
 * is a function of the utterance's frame list alone: not of its noise seed, the mode, the layout, the planner's choices or of whether the
 * batch has been synthesised; utterances that share a list share their source.
 * Framewise columns of speechPlayer_batch_exportSource, at the steps phase + j * hop:
 */
#define SPEECHPLAYER_SOURCE_F0            0   /* hz(t) */
#define SPEECHPLAYER_SOURCE_PHASE         1   /* P(t) */
#define SPEECHPLAYER_SOURCE_VIBRATO_PHASE 2   /* V(t) */
#define SPEECHPLAYER_SOURCE_CYCLE         3   /* C(t) */
#define SPEECHPLAYER_SOURCE_OPEN          4   /* 1 if P(t) >= glottalOpenQuotient(t), else 0 (a NaN compares false) */
#define SPEECHPLAYER_SOURCE_WAVE          5   /* (P(t) * 2 - 1) * voiceAmplitude(t): the reference's glottal wave before turbulence and
                                                 aspiration (src/speechWaveGenerator.cpp:81-83) */
#define SPEECHPLAYER_SOURCE_COLUMNS       6
/*
 * The epoch table has one entry per sample with epoch(t), in time order, four float64 values each:
 *   sample    t
 *   instant   t - P(t) / (hz(t) / sr), both plain IEEE divisions, t as a double: the sub-sample time of the wrap
 *   f0        hz(t)
 *   gain      voiceAmplitude(t) * preFormantGain(t); zero: the cycle is inaudible (a caller who wants voiced pitch marks filters on it)
 */
#define SPEECHPLAYER_EPOCH_COLUMNS 4
/* The source columns of chosen utterances into caller-owned device memory on the caller's stream.  Arguments, formats (0 float64,
 * 1 float32 rounded to nearest), packing, return value, refusals and event ordering are exactly those of speechPlayer_batch_exportTracks,
 * with columns 0 .. 5: valid as soon as the set call has returned, no synthesis launch, no host wait; the next set call waits for the
 * exports in flight and the seventeenth export in flight waits for the first.  One wavefront walks each distinct frame list the rows
 * speak -- one lane from option "source_lane_lists" (default 12288) lists up; the same bits -- and leaves 48 bytes per (list, step) in
 * a table; an export whose table would exceed option "source_table_mb" (default 256) proceeds in pieces of utterances, and exports
 * that use the table follow one another on the device. */
long long speechPlayer_batch_exportSource(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const int* columns, int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride, void* stream);
/* Epochs of every chosen utterance (utterances NULL: all) into counts[] (may be NULL).  The first call after a set call runs a counting
 * walk over the batch's lists on the engine's own stream and waits for it on the host (it downloads the counts); they are kept until
 * the next set call.  Returns the number of utterances, -1 when refused (no batch, an utterance number outside the batch). */
long long speechPlayer_batch_epochCounts(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, long long* counts);
/* The epoch table of chosen utterances, float64 [row][epoch][4], into caller-owned device memory on the caller's stream.
 *   rowStride   > 0: rowStride entries per row, `pad` in every column past the row's count; below the largest count it is refused;
 *               0: the rows back to back
 *   capacity    elements (doubles) deviceOut can take; fewer than the export needs is refused
 * Contract as speechPlayer_batch_exportUnits: returns the elements written (0 writes nothing and needs no buffer), -1 on error; ordered
 * by events like speechPlayer_batch_exportSource, except that the first call after a set call waits on the host for the counts
 * (speechPlayer_batch_epochCounts).  Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, an utterance number outside the
 * batch, rowStride < 0 or below the largest count, capacity below the elements needed, an output that is not device memory of the batch's
 * device, misaligned or too small. */
long long speechPlayer_batch_exportEpochs(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	void* deviceOut, long long rowStride, double pad, long long capacity, void* stream);
/*
 * The vocal-tract frequency response of a batch: the spectral envelope -- the frequency response of the filter network that the track
 * values configure on each sample, the cascade branch (N0, NP, r6 .. r1) and the parallel branch (p1 .. p6 with parallelBypass; reference
 * src/speechWaveGenerator.cpp:139-182).  For utterance u of a set batch at sample rate sr let cur(t) be the frame
 * speechPlayer_batch_exportTracks defines for sample t, its quirks included.  For a frequency f (Hz, any finite double):
 *   w = 6.283185307179586 * f / sr;   c1 = cos w, s1 = sin w, c2 = cos 2w, s2 = sin 2w (the C library's, made once per bin on the host);
 *   z1 = c1 - i s1, z2 = c2 - i s2
 *   (a, b, c)_r = coefficient_finish(coefficient_parts(cf, cb), anti, cf) of each of the 14 resonators from cur(t): the functions the
 *       synthesis kernels call (exp and cos of klatt_math.h inside their validated range)
 * and, every operation a separately rounded binary64 operation, complex products written out in real arithmetic
 * ((x y).re = x.re y.re - x.im y.im, (x y).im = x.re y.im + x.im y.re; sums and products from left to right):
 *   pole resonator   H_r = 0 when a_r == 0: its output is identically zero from a fresh state -- the all-zero frame of sample 0 and of
 *                    silence phonemes (f = bw = 0 gives a = 0 exactly).  Otherwise, with D = 1 - b_r z1 - c_r z2, i.e.
 *                    D.re = 1 - b c1 - c c2, D.im = b s1 + c s2:   q = a / (D.re D.re + D.im D.im) by IEEE division,
 *                    H_r = (q D.re, -(q D.im)).  A pole on a bin gives +-inf or NaN, and that is the answer.
 *   anti-resonator   H_N0 = a + b z1 + c z2 = (a + b c1 + c c2, -(b s1 + c s2)): always the FIR form; with cfN0 == 0 the coefficients are
 *                    the non-inverted ones (src/speechWaveGenerator.cpp:120, :133)
 *   cascade          T = H_N0 H_NP;  X = ((1 + (T.re - 1) caNP) 0.5, (T.im caNP) 0.5);  C = X H_6 H_5 H_4 H_3 H_2 H_1, the factors applied
 *                    in that order (:148-156)
 *   parallel         S = sum_{k = 1 .. 6} ((H_pk.re - 1) pa_k, H_pk.im pa_k), from zero;
 *                    P = ((S.re + (1 - S.re) parallelBypass) 0.5, (S.im + (0 - S.im) parallelBypass) 0.5)      (:171-179)
 *   gain != 0        both multiplied, component by component, by g = preFormantGain(t) * outputGain(t)
 * It is the frozen-time response of cur(t): the network with the coefficients of that one sample held for ever.  It does not depend on
 * voicePitch, the noise seed, the mode, the layout, the planner's choices or on whether the batch has been synthesised; utterances that
 * share a frame list share it.  Non-finite parameters propagate by IEEE arithmetic and give unspecified values, never a fault.
 * Kinds, in any order, repeats allowed:
 */
#define SPEECHPLAYER_RESPONSE_CASCADE_RE   0
#define SPEECHPLAYER_RESPONSE_CASCADE_IM   1
#define SPEECHPLAYER_RESPONSE_CASCADE_MAG  2   /* sqrt(re * re + im * im) */
#define SPEECHPLAYER_RESPONSE_CASCADE_DB   3   /* 20 * log10(MAG): -inf at 0 */
#define SPEECHPLAYER_RESPONSE_PARALLEL_RE  4
#define SPEECHPLAYER_RESPONSE_PARALLEL_IM  5
#define SPEECHPLAYER_RESPONSE_PARALLEL_MAG 6
#define SPEECHPLAYER_RESPONSE_PARALLEL_DB  7
#define SPEECHPLAYER_RESPONSE_KINDS        8
/* Host only, touches no device (like speechPlayer_planTimeline): the response of nFrames plain frames at sampleRate, by the definition
 * above with cur = the frame, out[frame][kind][bin] float64 -- the product's own CPU statement of the definition (a voice designer plots
 * one phoneme with it; the device path is held to it, bit for bit but for log10).  frequencies[nFrequencies]: 1 .. 4096 finite values.
 * Returns the elements written (0 for nFrames == 0), -1 on bad arguments. */
long long speechPlayer_frameResponse(const speechPlayer_frame_t* frames, long long nFrames, int sampleRate, const double* frequencies,
	int nFrequencies, const int* kinds, int nKinds, int gain, double* out);
/* The response of chosen utterances into caller-owned device memory on the caller's stream: element (i, j, q, k) of [row][step][kind][bin]
 * is kind kinds[q] of utterance utterances[i] at sample phase + j * hop and frequency frequencies[k].  frequencies is a HOST array,
 * 1 <= nFrequencies <= 4096; the library computes the four twiddles per bin on the host, so that the device and
 * speechPlayer_frameResponse use the same bits, and uploads them in the export's stream order.  Steps, rowStride (in steps, zeros past
 * the end), packing, format (0 float64, 1 float32 rounded to nearest), return value, device-memory checks, event ordering and the
 * sixteen-in-flight rule are exactly those of speechPlayer_batch_exportTracks: valid as soon as the set call has returned, no synthesis
 * launch, no host wait; the next set call waits for the exports in flight.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, a kind outside 0 .. 7, nKinds <= 0, nFrequencies outside
 * 1 .. 4096, a NULL or non-finite frequency, hop <= 0, phase < 0, an unknown format, an utterance number outside the batch, a rowStride
 * below the largest step count, an output that is not device memory of the batch's device, misaligned or too small. */
long long speechPlayer_batch_exportResponse(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const double* frequencies, int nFrequencies, const int* kinds, int nKinds, int gain, long long hop, long long phase,
	void* deviceOut, int format, long long rowStride, void* stream);
/*
 * The signal stems of a batch: what the synthesiser computes on every sample between the frame and the PCM -- the excitation that
 * enters the cascade and its periodic and aperiodic parts, the frication that enters the parallel bank, the outputs of the two filter
 * branches and the mixed sample before it is clipped and truncated to int16.  For utterance u of a set batch, of length L, with noise
 * seed s, at sample rate sr:
 *   cur(t)   the frame speechPlayer_batch_exportTracks defines for sample t, its quirks included
 *   P(t)     the glottal phase speechPlayer_batch_exportSource defines
 *   n(k)     value k of the utterance's noise stream (seed s): a 32-bit linear congruential generator whose start and increment come
 *            from the seed, value k = state k + 1 shifted right by one, 0 .. 2^31 - 1; u(k) = n(k) / 2147483647, correctly rounded
 *   fourteen resonators in the order N0, NP, c6 .. c1, p1 .. p6, each with memories z1 = z2 = 0 at t = -1 and, on sample t, the
 *            coefficients (a, b, c)_r(t) = coefficient_finish(coefficient_parts(cf_r(t), cb_r(t)), r == N0, cf_r(t)) of cur(t): the
 *            functions the synthesis kernels call and speechPlayer_batch_exportResponse names (speechPlayer_resonatorCoefficients
 *            states them on the host)
 *   A(-1) = F(-1) = 0
 * and, every operation a separately rounded binary64 operation, in this order (reference src/speechWaveGenerator.cpp:72-86, :147-180,
 * :203-208):
 *   A(t)       = u(2t) + 0.75 A(t-1);                      asp = A(t) 0.2
 *   turb       = asp voiceTurbulenceAmplitude;             turb = turb 0.01 unless P(t) >= glottalOpenQuotient
 *   VOICE      = ((P(t) 2 - 1) + turb) voiceAmplitude
 *   ASPIRATION = asp aspirationAmplitude
 *   SOURCE     = ASPIRATION + VOICE                        (what VoiceGenerator::getNext returns)
 *   x          = (SOURCE preFormantGain) 0.5
 *   n0 = res_N0(x) [its memory takes the input];  np = res_NP(n0);  o = hold_lerp(x, np, caNP)
 *   o          = res_c6(o) ... res_c1(o)                   res(in) = (a in + b z1) + c z2;  z2 = z1;  z1 = the output
 *   CASCADE    = o
 *   F(t)       = u(2t+1) + 0.75 F(t-1)
 *   FRICATION  = F(t) 0.3 fricationAmplitude
 *   y          = (FRICATION preFormantGain) 0.5
 *   par        = sum_{k = 1 .. 6} (res_pk(y) - y) pa_k, from zero, left to right;   PARALLEL = hold_lerp(par, y, parallelBypass)
 *   OUTPUT     = ((CASCADE + PARALLEL) outputGain) 4000    (before clipping and truncation)
 * hold_lerp(from, to, r) is `from` when `to` is NaN, else from + (to - from) r (reference src/utils.h:20-23).  The sample the reference
 * writes is (int)max(min(OUTPUT, 32000), -32000) with windows.h's min / max, so NaN becomes 32000: in MODE_EXACT that is the batch's
 * PCM, bit for bit.  The stems are ALWAYS this MODE_EXACT arithmetic: a function of the utterance's frames and seed alone, not of the
 * batch's mode, layout, planner choices or of whether it has been synthesised.  In MODE_FAST the PCM may differ from the truncated OUTPUT
 * by that mode's stated tolerance.  Non-finite parameters propagate by IEEE arithmetic, never a fault.
 * Columns, in any order, repeats allowed:
 */
#define SPEECHPLAYER_STEM_VOICE      0
#define SPEECHPLAYER_STEM_ASPIRATION 1
#define SPEECHPLAYER_STEM_SOURCE     2
#define SPEECHPLAYER_STEM_FRICATION  3
#define SPEECHPLAYER_STEM_CASCADE    4
#define SPEECHPLAYER_STEM_PARALLEL   5
#define SPEECHPLAYER_STEM_OUTPUT     6
#define SPEECHPLAYER_STEM_COLUMNS    7
/* The stems of chosen utterances into caller-owned device memory on the caller's stream, PLANAR: [row][column][sample] of float64
 * (format 0: the value itself) or float32 (format 1: rounded to nearest).  utterances, nUtterances, deviceOut and stream as
 * speechPlayer_batch_exportPcm's (any order, repeats allowed -- a repeated utterance is computed again; NULL: all).
 *   rowStride   > 0: column q of row i starts at element (i * nColumns + q) * rowStride, and elements past the utterance's end are 0; a
 *               stride below the longest chosen utterance is refused;
 *               0: the rows back to back, row i taking nColumns * L_i elements, column after column
 * Returns the number of elements written (0 writes nothing and needs no buffer), -1 on error.  Event ordering, the sixteen-in-flight
 * rule and the device-memory checks are exactly those of speechPlayer_batch_exportTracks: valid as soon as the set call has returned
 * (whichever set call it was), no synthesis launch, no host wait; the next set call waits for the exports in flight.  One lane computes
 * each row, the rows sorted by length; a 16-byte aligned buffer is written with 16-byte stores wherever a row's segment is aligned.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, a column outside 0 .. 6, nColumns <= 0, an unknown format, a
 * negative rowStride or one below the longest chosen utterance, an utterance number outside the batch, an output that is not device
 * memory of the batch's device, misaligned to the element or too small. */
long long speechPlayer_batch_exportStems(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const int* columns, int nColumns, void* deviceOut, int format, long long rowStride, void* stream);
/* Host only, touches no device: the resonator coefficients abc[n][3] = (a, b, c) of n (frequency, bandwidth) pairs at sampleRate, the
 * product's CPU statement of coefficient_finish(coefficient_parts(frequency, bandwidth), anti, frequency) -- the functions
 * speechPlayer_frameResponse uses.  anti != 0: the anti-resonator's coefficients (inverted unless the frequency is 0; reference
 * src/speechWaveGenerator.cpp:112-127).  With |pi bandwidth / sampleRate| <= 700 and |2 pi frequency / sampleRate| <= 1e4 these are
 * the device's bits (exp and cos of klatt_math.h); outside that range the C library's exp and cos are used, as the device uses its
 * library's, and the bits may differ.  Returns n, -1 on bad arguments (n < 0, sampleRate <= 0, a NULL array with n > 0). */
long long speechPlayer_resonatorCoefficients(const double* frequency, const double* bandwidth, long long n, int anti, int sampleRate,
	double* abc);
/*
 * The STFT and band (mel) spectrogram of a batch's PCM, on the step grid of the other exports.  For utterance u of a batch that has been
 * synthesised since it was set, of length L and int16 PCM s(t):
 *   steps     step j is centred on sample c = phase + j * hop; an utterance has ceil((L - phase) / hop) steps (0 when L <= phase): the
 *             grid of speechPlayer_batch_exportTracks, row for row
 *   frame     x[i] = (float)s(c - nFft/2 + i) / 32767.0f for i = 0 .. nFft-1 (the bits of speechPlayer_batch_exportPcm's format 1); a
 *             sample outside 0 .. L-1 is +0 (torch.stft's center=True, pad_mode="constant"); the pool's padding and the neighbouring
 *             utterance are never read as signal
 *   window    window[nFft], a HOST array of doubles, each rounded to float32 once; NULL: the periodic Hann 0.5 - 0.5 cos(2 pi i / nFft),
 *             evaluated in binary64 on the host.  xw[i] = x[i] * w[i], one float32 multiplication
 *   transform X[k] = sum_i xw[i] exp(-2 pi i k / nFft) for k = 0 .. nFft/2, computed in float32 by the functions of csrc/klatt_spectrum.h,
 *             which the host and the device compile from one source: a half-length complex radix-2 transform of the even / odd samples
 *             and an unpacking pass, every operation rounded separately (no fused multiply-add), twiddles made once on the host in
 *             binary64, rounded to float32 and uploaded in the export's stream order.  The definition is those function bodies;
 *             speechPlayer_pcmSpectrogram executes them in a plain loop.  nFft is a power of two in 64 .. 4096
 *   bin       p = re * re + im * im in float32 (two products, one sum); power 2: v = p; power 1: v = (float)sqrt((double)p), the binary64
 *             square root correctly rounded on both sides
 *   bands     bank[nBands][nFft/2 + 1], a HOST array of doubles, each rounded to float32; NULL: the bands are the bins.  Of every band the
 *             first and last non-zero column are found on the host; band_b = sum of w[b][k] * v[k] over that column range in ascending k,
 *             each term one product and one sum in float32, from +0; a band without a non-zero weight is +0
 *   log       logScale == 0: the linear value.  Otherwise logScale * log10(max((double)value, floor)) in binary64, floor > 0 required:
 *             10 gives power dB, 20 magnitude dB, 2.302585092994046 the natural logarithm
 *   output    element (i, j, b) of [row][step][band]; format 0 float64 (widens linear values exactly), 1 float32 rounded to nearest
 * Unlike the exports of the batch "as set" above, the result is a function of the batch's PCM: it depends on the mode and, in MODE_FAST,
 * on whatever that mode's tolerance allows; it needs a synthesis launch.
 *
 * Host only, touches no device (like speechPlayer_frameResponse): the definition above on `length` samples of plain PCM,
 * out[step][band] float64 -- the product's own CPU statement, which the device path is held to bit for bit on linear values (log10 is
 * each side's library call).  Returns steps * bands (bands = nBands with a bank, nFft/2 + 1 without), -1 on bad arguments: those of the
 * refusal list below that concern the request, length < 0, a NULL pcm with length > 0, a NULL out with steps > 0. */
long long speechPlayer_pcmSpectrogram(const sample* pcm, long long length, int nFft, long long hop, long long phase, const double* window,
	const double* bank, int nBands, int power, double logScale, double floor, double* out);
/* The spectrogram of chosen utterances into caller-owned device memory on the caller's stream.  utterances (any order, repeats allowed,
 * NULL: all), rowStride (in steps, +0 past the utterance's end; 0: the rows back to back), the return value (elements written; 0 writes
 * nothing and needs no buffer), the device-memory and alignment checks (16-byte alignment takes the vector stores) and the
 * sixteen-in-flight rule are those of speechPlayer_batch_exportTracks.  Ordering is that of speechPlayer_batch_exportPcm, by events and
 * without a host wait: the export runs on `stream` behind the batch's last synthesis launch on all its streams, and the batch's next
 * launch waits on the device for the export before it overwrites the pool.  One wavefront computes each step (csrc/klatt_spectrum.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, a batch that has not been synthesised since it was set, nFft not a
 * power of two in 64 .. 4096, hop <= 0, phase < 0, power outside {1, 2}, nBands <= 0 with a bank, a non-finite window or bank value,
 * logScale != 0 with floor <= 0, a non-finite logScale or floor, an unknown format, an utterance number outside the batch, a rowStride
 * below the largest step count, an output that is not device memory of the batch's device, misaligned to the element or too small.
 * Out of scope: live handles through this export (the last nFft - 1 samples would have to persist across pulls: "Signal stages that keep
 * a window", below, keep them -- speechPlayer_batch_stageSpectrogram). */
long long speechPlayer_batch_exportSpectrogram(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int nFft,
	long long hop, long long phase, const double* window, const double* bank, int nBands, int power, double logScale, double floor,
	void* deviceOut, int format, long long rowStride, void* stream);
/*
 * A batch's PCM at another sample rate: a polyphase windowed-sinc resampler.  For an utterance of Lin samples of int16 PCM s(t), the
 * source rate sr (the batch's) and the target rate out:
 *   ratio     g = gcd(sr, out), up = out / g, down = sr / g.  Lout = ceil(Lin * up / down) in 64-bit integers, 0 when Lin is 0.  Output
 *             sample m lies at source time m * down / up (in source samples): grids and labels of the other exports are at the SOURCE rate
 *   filter    c = rolloff * min(1, up / down), the cut-off as a fraction of the source Nyquist frequency; Wd = zeros / c, the half-width
 *             in source samples; Z = ceil(Wd); taps = 2 Z, with offsets i = -Z+1 .. Z
 *   table     h[p][k] for p = 0 .. up-1 and k = 0 .. taps-1, with i = k - Z + 1 and t = i - p / up:  h = c * sinc(c t) * w(t), where
 *             sinc(x) = sin(pi x) / (pi x) and is 1 at 0, and w(t) = 0 when |t| >= Wd.  window 0 (Hann): w(t) = cos^2(pi t / (2 Wd)).
 *             window 1 (Kaiser): w(t) = I0(beta * sqrt(1 - (t/Wd)^2)) / I0(beta), I0 by its power series.  The table is evaluated in
 *             binary64 on the host, rounded to float32 once and used by both sides
 *   input     x[n] = (float)s(n) / 32767.0f (the bits of speechPlayer_batch_exportPcm's format 1); a sample outside 0 .. Lin-1 is +0; the
 *             pool's padding and the neighbouring utterances are never read as signal
 *   output    for m = 0 .. Lout-1: n0 = floor(m * down / up) and p = (m * down) mod up, both in 64-bit integers; y[m] is the sum over
 *             k ascending, starting from +0, of x[n0 + k - Z + 1] * h[p][k], each term one float32 product and one float32 sum, no
 *             fused multiply-add.  The definition is the function bodies of csrc/klatt_resample.h, which the host and the device
 *             compile from one source; speechPlayer_pcmResample executes them in a plain loop
 *   format 1  float32: y[m]
 *   format 0  int16: q = y * 32767.0f, one float32 product; 32767 when q >= 32767, -32768 when q <= -32768, otherwise rintf(q), rounded
 *             to nearest even.  Clipping does happen: the filter overshoots on full-scale noise
 *   equal     out == sr does no filtering: the result is speechPlayer_batch_exportPcm's output exactly
 * Like the spectrogram, and unlike the exports of the batch "as set", the result is a function of the batch's PCM: it depends on the
 * mode and, in MODE_FAST, on whatever that mode's tolerance allows; it needs a synthesis launch.
 * Out of scope: live handles through this export (resampling across pulls needs filter state: "Signal stages", below, keep it --
 * speechPlayer_batch_stageResample); NodePlayer, which reaches the export through
 * speechPlayer_node_part; a label grid at the target rate (see "ratio" for where output sample m lies).  A spectrogram at the target
 * rate is speechPlayer_batch_exportSpectrogramOf of this export's output ("The exports of a signal", below).
 *
 * Refused by all of the entry points below with SPEECHPLAYER_ERR_ARGUMENT and nothing written: a rate <= 0, zeros < 1, rolloff outside
 * (0, 1] or not finite, an unknown window, Kaiser with beta not finite or negative, up > 4096, taps > 1024, up * taps > 2^20.
 *
 * Host only, touches no device: Lout for `length` samples (-1: length < 0 or a rate <= 0). */
long long speechPlayer_resampledLength(long long length, int srcRate, int dstRate);
/* Host only: the float32 table widened to double, table[up][taps]; *up, *down, *taps (each may be NULL).  Returns up * taps; a NULL
 * table only sizes; -1 on a refused request or a capacity below up * taps.  (With equal rates it is the filter the formulas give, which the
 * resampler does not apply.) */
long long speechPlayer_resampleKernel(int srcRate, int dstRate, int zeros, double rolloff, int window, double beta, int* up, int* down, int* taps,
	double* table, long long capacity);
/* Host only: the definition above on `length` samples of plain PCM -- the product's own CPU statement, which the device path is held to
 * bit for bit.  out: float[Lout] (format 1) or int16[Lout] (format 0).  Returns Lout; a NULL out only sizes; -1 on a refused request, an
 * unknown format, length < 0 or above 2^44, a NULL pcm with length > 0, a capacity below Lout. */
long long speechPlayer_pcmResample(const sample* pcm, long long length, int srcRate, int dstRate, int zeros, double rolloff, int window, double beta,
	int format, void* out, long long capacity);
/* The chosen utterances' PCM at outRate into caller-owned device memory on the caller's stream.  utterances (any order, repeats allowed,
 * NULL: all), the rows (rowStride > 0: padded rows, +0 past each row's Lout; 0: the rows back to back), the return value (elements
 * written; 0 writes nothing and needs no buffer), the device-memory checks and the sixteen-in-flight rule are those of
 * speechPlayer_batch_exportPcm, and so is the ordering, by events and without a host wait: the export runs on `stream` behind the batch's
 * last synthesis launch on all its streams, and the batch's next launch waits on the device for the export before it overwrites the
 * pool.  A workgroup takes tiles of kResampleTile = 1024 consecutive outputs of one row (csrc/klatt_resample.h); the table stays on the
 * batch until the parameters change and is uploaded in the export's stream order.  An output aligned to 16 bytes or only to its element
 * takes 16-byte stores wherever a run of outputs covers an aligned 16 bytes.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: the list above, no batch, a batch that has not been synthesised since it
 * was set, an unknown format, an utterance number outside the batch, a rowStride below the longest output row, an output that is not
 * device memory of the batch's device, misaligned to the element or too small. */
long long speechPlayer_batch_exportResampled(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int outRate, int zeros,
	double rolloff, int window, double beta, void* deviceOut, int format, long long rowStride, void* stream);
/*
 * A batch's PCM convolved with impulse responses: an FIR filter per row -- a room, a channel, a microphone.  For a row whose utterance
 * has L samples of int16 PCM s(t), and an impulse response h[0 .. K-1] of float32:
 *   input     x[n] = (float)s(n) / 32767.0f (the bits of speechPlayer_batch_exportPcm's format 1); a sample outside 0 .. L-1 is +0; the
 *             pool's padding and the neighbouring utterances are never read as signal
 *   length    tail = 1: Lout = L + K - 1, the full convolution, reverberant tail included.  tail = 0: Lout = L, the first L outputs, so
 *             the label grids of the other exports apply unchanged.  Output sample m lies at source sample m: whatever delay the response
 *             has is the caller's
 *   output    for m = 0 .. Lout-1: acc = +0; for k = 0 .. K-1 ascending acc = fmaf(x[m - k], h[k], acc), each step ONE correctly rounded
 *             binary32 fused multiply-add with gradual underflow; y[m] = acc + 0.0f.  The definition is the function bodies of
 *             csrc/klatt_convolve.h (conv_step, conv_finish), which the host and the device compile from one source;
 *             speechPlayer_pcmConvolve executes them in a plain loop
 *   format 1  float32: y[m]
 *   format 0  int16: the resampler's conversion of y[m] (one float32 product by 32767, clipped to 32767 and -32768, rintf)
 *   responses every h[k] is finite and |h[k]| <= 2^32, refused otherwise: with K <= kConvolveMaxTaps = 65536 and |x| <= 32768 / 32767 no
 *             sum overflows, so no NaN appears whose bits would differ between host and device
 * The resampler forbids fusing; this definition demands it: it halves the instruction count of a loop that is the whole cost at
 * thousands of taps; fmaf is exact by the C standard on the host, whatever the build flags; the device's v_fma_f32 / v_pk_fma_f32 are
 * the same operation; and an f32 MFMA on this part is documented as bitwise an fmaf chain, so a later matrix-core kernel could meet the
 * same bits (it is not part of this export).
 * Lemma.  For finite operands, inserting or removing terms whose product is +-0 -- samples outside the utterance, zero taps, the zero
 * padding of a tap block -- does not change y[m].  A +-0 product added to a nonzero acc returns acc; added to a zero acc it returns a
 * zero; a zero acc of either sign followed by a nonzero product p returns RN(p).  So two such sequences agree at every step except
 * possibly in the sign of a zero, and the closing + 0.0f makes that +0.  This is what lets the kernel skip tap blocks that lie wholly
 * outside the signal, pad blocks to a multiple of four taps and stage masked inputs.
 * Like the resampler, the result is a function of the batch's PCM: it depends on the mode and, in MODE_FAST, on whatever that mode's
 * tolerance allows; it needs a synthesis launch.
 * Out of scope: live handles through this export (the last K - 1 samples would have to persist across pulls: "Signal stages that keep a
 * window", below, keep them -- speechPlayer_batch_stageConvolve); NodePlayer, which reaches the export through speechPlayer_node_part;
 * per-row gains and wet/dry mixes (put them in the response); FFT or MFMA formulations.  A spectrogram or resampling of the convolved
 * signal is speechPlayer_batch_exportSpectrogramOf / exportResampledOf of this export's output ("The exports of a signal", below).
 *
 * Host only, touches no device: the definition above on `length` samples of plain PCM and one response of `taps` values -- the statement
 * the device is held to bit for bit.  out: float[Lout] (format 1) or int16[Lout] (format 0).  Returns Lout; a NULL out only sizes; -1 on
 * tail not 0 or 1, a NULL ir, taps < 1 or above 65536, a tap that is not finite or above 2^32 in magnitude, an unknown format,
 * length < 0 or above 2^44, a NULL pcm with length > 0, a capacity below Lout. */
long long speechPlayer_pcmConvolve(const sample* pcm, long long length, const float* ir, long long taps, int tail, int format, void* out,
	long long capacity);
/* The chosen utterances' PCM, row i convolved with response irOf[i], into caller-owned device memory on the caller's stream.  The nIr
 * responses lie back to back in HOST memory: response j is ir[irStart[j] .. irStart[j+1]-1] (irOf NULL: nIr must be 1).  irOf is per ROW,
 * not per utterance: with repeats in `utterances`, one utterance goes through several rooms in one call.  utterances (any order,
 * repeats allowed, NULL: all), the rows (rowStride > 0: padded rows, +0 past each row's Lout; 0: the rows back to back), the return value
 * (elements written; 0 writes nothing and needs no buffer), the device-memory checks, the sixteen-in-flight rule and the ordering by
 * events are those of speechPlayer_batch_exportPcm.  The responses cross the link with the call's staging block, like the row table, and
 * are not kept on the batch (no new ordering state; at most kConvolveMaxTable = 2^20 taps, 4 MB, which the staging path takes as it
 * is).  A workgroup takes tiles of kConvolveTile = 1024 consecutive outputs of one row, and the taps in blocks of kConvolveBlock = 1024
 * (csrc/klatt_convolve.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: no batch, a batch that has not been synthesised since it was set, an
 * unknown format, rowStride < 0 or below the longest output row, an utterance number outside the batch, an output that is not device
 * memory of the batch's device, misaligned to the element or too small; tail not 0 or 1; nIr < 1; a NULL ir or irStart; irStart not
 * starting at 0 or not increasing (a response of 0 taps); a response of more than 65536 taps; more than 2^20 taps in all; an irOf[i]
 * outside 0 .. nIr-1; irOf NULL with nIr != 1; a tap that is not finite or above 2^32 in magnitude (the message gives response and tap). */
long long speechPlayer_batch_exportConvolved(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const float* ir,
	const long long* irStart, long long nIr, const long long* irOf, int tail, void* deviceOut, int format, long long rowStride, void* stream);
/*
 * A batch's PCM mixed with noise and other utterances at set levels: additive noise at a chosen signal-to-noise ratio, babble, two-talker
 * mixtures -- the other half of an augmentation recipe beside speechPlayer_batch_exportConvolved.  For a row whose utterance has L samples
 * of int16 PCM s(t):
 *   input     x[n] = (float)s(n) / 32767.0f (the bits of speechPlayer_batch_exportPcm's format 1).  The output has L samples, on the grid of
 *             the other exports; there is no tail
 *   sources   a CLIP of the batch's noise bank (speechPlayer_batch_setNoiseBank): float32 c[0 .. N-1], 1 <= N < 2^31, every value finite and
 *             at most 2^16 in magnitude; or an UTTERANCE of the same batch, x_u[n] = (float)s_u(n) / 32767.0f, N = L_u -- it may be the
 *             row's own
 *   powers    of an utterance: S_u = sum s_u(n)^2 as an exact unsigned 64-bit integer (order-free: any reduction gives the same bits;
 *             speechPlayer_batch_exportPower hands it out) and P_u = (double)S_u / (double)L_u / 1073676289.0, 0 for L_u = 0.  Of a clip:
 *             P_c = (sum over n ascending of (double)c[n] * (double)c[n]) / N, computed once on the host when the bank is set and kept
 *             with it (speechPlayer_batch_noiseBank).  Both are WHOLE-SIGNAL mean squares, silences included
 *   placement term j with loop = 1: v_j[m] = src[(offset + m) mod N], 0 <= offset < N.  loop = 0: v_j[m] = src[m - offset] where
 *             0 <= m - offset < N, else +0; |offset| <= 2^44; a negative offset skips the source's beginning
 *   level     levelKind = 1: g_j = (float)level, finite, |level| <= 2^32.  levelKind = 0: level is an SNR in dB, finite, |level| <= 200;
 *             ratio = pow(10.0, level / 10.0) is evaluated on the HOST for both statements, and g_j = mix_gain(Ps, Pv, ratio) =
 *             (Ps > 0 && Pv * ratio > 0) ? (float)fmin(sqrt(Ps / (Pv * ratio)), 4294967296.0) : 0.0f -- one binary64 product, one
 *             quotient and one square root, each IEEE on both sides.  Ps is the power of the row's own utterance at gain 1, whatever
 *             speechGain is; a silent row or a silent source gives gain 0
 *   output    acc = speechGain * x[m], one binary32 product (speechGain finite, at most 2^32 in magnitude; NULL: 1); for j ascending
 *             acc = fmaf(v_j[m], g_j, acc); y[m] = acc + 0.0f.  Format 1 is y[m], format 0 the resampler's int16 conversion of it.  With
 *             at most kMixMaxTerms = 64 terms per row no sum overflows under the bounds above.  The convolution's Lemma holds: a term whose
 *             product is +-0 may be dropped without changing a bit, so the kernel skips a term that lies wholly outside a tile
 * The definition is the function bodies of csrc/klatt_mix.h (mix_power, mix_gain, mix_source_index; conv_step and conv_finish of
 * csrc/klatt_convolve.h), which the host and the device compile from one source; speechPlayer_pcmMix executes them in a plain loop.
 * The result is a function of the batch's PCM: it needs a synthesis launch, depends on the mode (in MODE_FAST on whatever that mode's
 * tolerance allows) and is ordered as speechPlayer_batch_exportPcm is.
 * Mixing onto a convolved or resampled signal -- noise at an SNR against the reverberant speech -- is speechPlayer_batch_exportMixedOf,
 * below: an SNR needs the row's power, which for a float32 signal has no order-free exact definition as the pool's integer sum is, so
 * host and device share a fixed reduction shape (csrc/klatt_sigpower.h).
 * Out of scope: a term from a different signal, or from the pool in a mix onto a signal; live handles; NodePlayer, which reaches the
 * export through speechPlayer_node_part; segment or active-speech (VAD-weighted) levels; loudness weighting; random draws of any kind --
 * clips, offsets and levels are the caller's.
 */
typedef struct {
	int kind;            /* 0 a clip of the noise bank, 1 an utterance of the batch */
	int levelKind;       /* 0 `level` is an SNR in dB, 1 a linear gain */
	long long source;    /* the clip's or the utterance's number */
	long long offset;
	double level;
	int loop;            /* 0 or 1 */
	int reserved;
} speechPlayer_mixTerm_t;
typedef struct {
	const void* data;
	long long length;
	int format;          /* 0 int16 (an utterance), 1 float32 (a clip) */
} speechPlayer_mixSource_t;
/* The batch's noise bank: nNoise clips back to back in HOST memory, clip k is noise[noiseStart[k] .. noiseStart[k+1]-1].  It is validated
 * and its clips' powers are computed on the host; the samples are kept in device memory.  At most 2^20 clips and 2^28 samples; nNoise = 0
 * frees it.  It survives set calls and synthesis launches and dies with the batch.  Replacing it waits for the exports that read the old
 * one; an export issued after the call returns reads the new one.  Returns 0, or -1 (SPEECHPLAYER_ERR_ARGUMENT, the bank as it was): no
 * batch, nNoise outside 0 .. 2^20, a NULL noise or noiseStart, noiseStart not starting at 0 or not increasing (a clip of no samples), more
 * than 2^28 samples, a value that is not finite or above 2^16 in magnitude (the message gives clip and sample). */
int speechPlayer_batch_setNoiseBank(speechPlayer_batch_t batch, const float* noise, const long long* noiseStart, long long nNoise);
/* The bank's clips: returns their number (0: no bank) and fills power[] (P_c) and length[] (each may be NULL) when it is <= capacity. */
long long speechPlayer_batch_noiseBank(speechPlayer_batch_t batch, double* power, long long* length, long long capacity);
/* S_u of the chosen utterances, one uint64 per row, into caller-owned device memory on the caller's stream: speechPlayer_batch_exportPcm's
 * contract (row selection, return value = rows written, device-memory checks, the sixteen-in-flight rule, ordering by events, no host
 * wait) over one element per row.  Lanes accumulate in 64 bits; one 64-bit atomic add per wavefront (csrc/klatt_mix.h: klatt_power). */
long long speechPlayer_batch_exportPower(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, void* deviceOut, void* stream);
/* The chosen utterances' PCM, row i mixed with its terms terms[termStart[i] .. termStart[i+1]-1] (termStart: n + 1 entries, CSR per ROW --
 * not per utterance: with repeats in `utterances`, one utterance gets several mixtures in one call; equal entries are a row with no terms),
 * into caller-owned device memory on the caller's stream.  speechGain: one per row (NULL: 1).  deviceGains: NULL, or device memory for
 * termStart[n] floats that receive the g_j actually applied -- the labels of the mixture.  utterances, the rows (rowStride > 0: padded
 * rows, +0 past each row's L; 0: the rows back to back), the return value (elements written; 0 writes nothing and needs no buffer), the
 * device-memory checks, the sixteen-in-flight rule, the ordering by events and the absence of host waits are those of
 * speechPlayer_batch_exportPcm; a call that names a clip also follows the other readers of the bank.  A workgroup takes tiles of
 * kMixTile = 1024 consecutive outputs of one row (csrc/klatt_mix.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written (the message names row and term): no batch, a batch that has not been
 * synthesised since it was set, an unknown format, rowStride < 0 or below the longest row, an utterance number outside the batch, an
 * output or deviceGains that is not device memory of the batch's device, misaligned to the element or too small; a NULL termStart, or one
 * that does not start at 0 or decreases; more than 64 terms in a row or 2^22 in a call; terms NULL where there are some; a kind or
 * levelKind other than 0 or 1, a loop other than 0 or 1; a clip with no bank set, or outside the bank; a source utterance outside the
 * batch; a looped term on a source of length 0 or with an offset outside 0 .. N-1; an offset above 2^44 in magnitude; a gain or speech
 * gain that is not finite or above 2^32 in magnitude; an SNR that is not finite or above 200 dB in magnitude. */
long long speechPlayer_batch_exportMixed(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const speechPlayer_mixTerm_t* terms, const long long* termStart, const float* speechGain, void* deviceGains, void* deviceOut, int format,
	long long rowStride, void* stream);
/* Host only, touches no device: the definition above on `length` samples of plain PCM (at most 2^33) -- the statement the device is held
 * to bit for bit.  A term's `source` indexes `sources`, whatever its kind: kind 0 names a float32 source (a clip: 1 .. 2^31 - 1 values,
 * each finite and at most 2^16 in magnitude), kind 1 an int16 one (an utterance: 0 .. 2^33 samples).  gains: NULL, or nTerms floats that
 * receive the g_j.  out: float[length] (format 1) or int16[length] (format 0).  Returns length; a NULL out only sizes (and fills gains);
 * -1 on the refusals above that apply (row 0), nTerms above 64, a source whose format does not fit the term's kind, a capacity below
 * length. */
long long speechPlayer_pcmMix(const sample* pcm, long long length, float speechGain, const speechPlayer_mixSource_t* sources, long long nSources,
	const speechPlayer_mixTerm_t* terms, long long nTerms, float* gains, int format, void* out, long long capacity);
/* The exports of a signal: the spectrogram, the resampler, the convolution, the mix and the power on rows of samples in the CALLER's
 * device memory, in place of the batch's pool -- what speechPlayer_batch_exportPcm, exportMixed, exportConvolved and exportResampled
 * return, so that the output of one goes into the next: the log-mel of reverberant speech in noise at 16 kHz is exportConvolved,
 * exportMixedOf, exportResampledOf, exportSpectrogramOf -- the speech through a room first, then the noise at an SNR measured against
 * the reverberant speech.
 * A signal is nRows rows of int16 or float32 samples from `data`.  Padded (rowStride > 0): row r starts at element r * rowStride and has
 * extent[r] <= rowStride samples.  Packed (rowStride 0): extent holds nRows + 1 ascending offsets from 0, row r is the elements
 * extent[r] .. extent[r + 1] - 1.  extent is HOST memory, read during the call.
 * The definitions are those of the three exports above with "the utterance's int16 PCM s(t), L samples" replaced by "the row's samples,
 * L of them": format 0 converts as the pool's samples are, x = (float)s / 32767.0f; format 1 takes x as it is, and every later operation
 * is unchanged.  Samples outside 0 .. L-1 are +0: a padded row's remainder and the neighbouring rows are never read as signal, whatever
 * bits they hold -- they are not loaded at all.  For a signal, equal rates in the resampler mean y[m] = x[m] (format 1) or its int16
 * conversion (format 0).  `rows` / `nRows` choose rows of the signal in any order, repeats allowed (NULL: all, in order) and play the
 * part `utterances` plays above: irOf is per OUTPUT row.  exportResampledOf takes the signal's rate, srcRate, since a signal has none of
 * its own; the batch's table is keyed by it.
 * Ordering    The export reads `data` on `stream`: ordering whatever produces the signal before it is the caller's job (on one stream
 *             it is automatic).  It does not read the pool: it does not wait for a synthesis launch, the batch's next launch does not
 *             wait for it, and it works on a batch that has never been set or is set but not synthesised -- the batch gives the device,
 *             the staging blocks and the resampler's table.  At most sixteen may be in flight per batch, shared with the exports of the
 *             batch "as set"; the seventeenth waits on the host for the oldest.  The resampler's table keeps its one order.
 * Values      The device equals the host statements below bit for bit (through log10: within its few ulp, as above) for finite
 *             samples of magnitude at most 2^16, the noise bank's bound: with K <= 65536 taps of magnitude at most 2^32 no sum
 *             overflows, and the convolution's Lemma, which needs finite operands, holds.  The device cannot check this without a pass
 *             over the data and does not.  Outside the bound the bits are unspecified; no sample's value ever steers an address.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written, beyond each export's own list: a NULL signal or an unknown format;
 * nRows < 0; rowStride < 0; a NULL extent with nRows > 0; a negative length or one above rowStride; packed offsets that do not start
 * at 0 or that decrease; a length above 2^44; data that is not device memory of the batch's device, misaligned to its element, or
 * whose allocation is smaller than the rows need (a signal whose rows are all empty is not read and may have no data); a row number
 * outside the signal; an output that overlaps the signal; srcRate <= 0.  The message names the row.
 * Limits      A row has at most 2^44 samples, a signal 2^60 elements, an output 2^50; tests/test_gpu_far_offsets.py (and
 *             tests/test_gpu_lpc.py and tests/test_gpu_tempo.py for the linear-prediction and tempo exports) runs every export past elements 2^31 and 2^32 of its output and
 *             of a signal, and past sample 2^31 of the pool (docs/KERNELS.md 4.22).
 * Out of scope: in a mix onto a signal, a term from a different signal or from the pool; live handles; NodePlayer beyond
 * speechPlayer_node_part; active-speech levels and loudness weighting; a fused kernel for the chain; float64 or float16 signals; label
 * grids at a resampled rate. */
typedef struct {
	const void* data;         /* device memory of the batch's device, aligned to its element */
	int format;               /* 0 int16: x = (float)s / 32767.0f, as the pool's samples; 1 float32: x as it is */
	int reserved;
	long long nRows;
	long long rowStride;      /* > 0: row r starts at r * rowStride and has extent[r] <= rowStride samples; 0: packed */
	const long long* extent;  /* HOST: nRows lengths (padded) or nRows + 1 ascending offsets from 0 (packed) */
} speechPlayer_signal_t;
/* speechPlayer_batch_exportSpectrogram, exportResampled and exportConvolved of chosen rows of `signal`: the remaining arguments, the
 * output's forms and the return value are theirs. */
long long speechPlayer_batch_exportSpectrogramOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int nFft, long long hop, long long phase, const double* window, const double* bank, int nBands, int power, double logScale, double floor,
	void* deviceOut, int format, long long rowStride, void* stream);
long long speechPlayer_batch_exportResampledOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int srcRate, int outRate, int zeros, double rolloff, int window, double beta, void* deviceOut, int format, long long rowStride, void* stream);
long long speechPlayer_batch_exportConvolvedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	const float* ir, const long long* irStart, long long nIr, const long long* irOf, int tail, void* deviceOut, int format, long long rowStride,
	void* stream);
/*
 * The power of a signal's row and the mix onto a signal.  For a row of L samples:
 *   int16     (format 0) the pool's definition: S = sum s^2 as an exact unsigned 64-bit integer, P = (double)S / (double)L / 1073676289.0.
 *             The pool handed back as an int16 signal gives the pool's bits
 *   float32   (format 1) sq(x) = (double)x * (double)x -- exact in binary64, so that fusing it into an FMA changes no bit.  Samples at
 *             index L or beyond are +0.  A BLOCK is kSigPowerBlock = 2048 consecutive samples, 256 LEAVES of 8 consecutive samples:
 *             leaf = ((((((sq0 + sq1) + sq2) + ...) + sq7), ascending; the block sum is the balanced binary tree over the 256 leaves in
 *             natural order, t[i] = t[2i] + t[2i+1], eight levels.  Q is the ascending sum of the block sums from +0.0; P = Q / (double)L,
 *             and P = 0 for L = 0
 *   Lemma     every addend is >= +0, and adding +0 to a non-negative binary64 changes no bit: absent samples, absent leaves and a
 *             short last block may be taken as zeros, and nothing past a row is loaded to fill them
 *   bound     the signal contract's: finite samples of magnitude at most 2^16; no sum overflows.  Outside it the bits are unspecified
 * Both are WHOLE-SIGNAL mean squares, silences included.  The definition is the function bodies of csrc/klatt_sigpower.h, which the host
 * and the device compile from one source; its error against the exact mean square is at most (16 + blocks) * 2^-53 * P.
 * speechPlayer_batch_exportPowerOf: P of the chosen rows, one binary64 per row, into caller-owned device memory: the contract of the
 * exports of a signal above over one element per row (the output may not overlap the signal).
 * speechPlayer_batch_exportMixedOf is speechPlayer_batch_exportMixed with "the utterance's int16 PCM" replaced by "the row's samples":
 * kind 0 is a clip of the batch's noise bank, as there, and follows the bank's order; kind 1 names A ROW OF THE SAME SIGNAL -- any row,
 * chosen or not, the row's own included --, whose power is the one above; Ps is the row's own power at gain 1; the output has the row's L
 * samples.  `rows` / `nRows` play the part `utterances` plays; termStart and speechGain are per OUTPUT row.  Its contract is that of the
 * exports of a signal: the caller orders the producer, it reads no pool and waits for no launch, works on a batch never set, takes a slot
 * of the sixteen in flight, and neither the output nor deviceGains may overlap the signal.  Only rows named by an SNR term (or by
 * exportPowerOf) are powered, each distinct row once per call; the block partials, 8 bytes per 2048 powered samples, live in the call's
 * staging slot, and a call whose powered rows take more than kSigPowerMaxBlocks = 2^24 blocks is refused.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what speechPlayer_batch_exportMixed refuses (but a batch not synthesised),
 * with "source ... is not a row of the signal" for a kind-1 source outside it; what the exports of a signal refuse; the cap above.
 */
long long speechPlayer_batch_exportPowerOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	void* deviceOut, void* stream);
long long speechPlayer_batch_exportMixedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	const speechPlayer_mixTerm_t* terms, const long long* termStart, const float* speechGain, void* deviceGains, void* deviceOut, int format,
	long long rowStride, void* stream);
/* Host only, touch no device: the statements the two are held to bit for bit.  speechPlayer_signalPower: P of `length` samples (at most
 * 2^33), int16 (inFormat 0) or float32 (inFormat 1), into *power; returns 0, or -1: an unknown inFormat, a bad length, a NULL power, a
 * float32 sample that is not finite or above 2^16 in magnitude.  speechPlayer_signalMix is speechPlayer_pcmMix on a signal's row: a
 * kind-1 term names a source of either format, a row, whose power is the one above; a kind-0 term names a float32 source, a clip
 * (1 .. 2^31 - 1 values, the clip's power).  Beyond speechPlayer_pcmMix's refusals it refuses an unknown inFormat and a float32 sample of
 * x outside the bound.  With int16 inputs throughout it equals speechPlayer_pcmMix bit for bit. */
int speechPlayer_signalPower(const void* x, int inFormat, long long length, double* power);
long long speechPlayer_signalMix(const void* x, int inFormat, long long length, float speechGain, const speechPlayer_mixSource_t* sources, long long nSources,
	const speechPlayer_mixTerm_t* terms, long long nTerms, float* gains, int format, void* out, long long capacity);
/* Host only, touch no device: speechPlayer_pcmSpectrogram, pcmResample and pcmConvolve on `length` samples of a signal's row, int16
 * (inFormat 0: their bits exactly) or float32 (inFormat 1) -- the same function bodies, and the statements the device is held to.  They
 * have the data, so beyond the refusals of speechPlayer_pcm* they refuse an unknown inFormat and a float32 sample that is not finite or
 * is above 2^16 in magnitude; the message gives the sample. */
long long speechPlayer_signalSpectrogram(const void* x, int inFormat, long long length, int nFft, long long hop, long long phase, const double* window,
	const double* bank, int nBands, int power, double logScale, double floor, double* out);
long long speechPlayer_signalResample(const void* x, int inFormat, long long length, int srcRate, int dstRate, int zeros, double rolloff, int window,
	double beta, int format, void* out, long long capacity);
long long speechPlayer_signalConvolve(const void* x, int inFormat, long long length, const float* ir, long long taps, int tail, int format, void* out,
	long long capacity);
/*
 * A batch's PCM, or a signal's rows, through cascades of second-order recursive (biquad, IIR) sections: pre-emphasis and de-emphasis, a
 * DC blocker, the telephone band, shelving and peaking EQ, a high-pass -- and the synthesiser's own building block, the resonator
 * (speechPlayer_resonatorCoefficients: y = a x + b y1 + c y2 is the section b0 = a, b1 = b2 = 0, a1 = -b, a2 = -c).  For a row of L
 * input samples and a filter of K sections (1 <= K <= kFilterMaxSections = 16), section j being five float32 values b0 b1 b2 a1 a2
 * (a0 = 1):
 *   input     x[n] = tile_x(s(n)): (float)s(n) / 32767.0f of an int16 sample (the bits of speechPlayer_batch_exportPcm's format 1), a
 *             float32 sample as it is; x[n] = +0 for n >= L; nothing outside the row is read as signal
 *   length    Lout = L + tail: tail >= 0 extra samples of zero input, the same for all rows, at most 2^20.  With tail = 0 the label grids
 *             of the other exports apply unchanged
 *   section   transposed direct form II, the states s1 = s2 = +0 at n = 0; na1 = -a1 and na2 = -a2 are exact negations made once.  For
 *             every sample, in this order, each line ONE correctly rounded binary32 operation with gradual underflow:
 *                 y  = fmaf(b0,  x, s1)
 *                 t  = fmaf(b1,  x, s2)
 *                 s1 = fmaf(na1, y, t)
 *                 v  = b2 * x
 *                 s2 = fmaf(na2, y, v)
 *             The y of section j is the x of section j + 1; after the last section out = y + 0.0f.  The definition is the function bodies
 *             of csrc/klatt_filter.h (filter_section, filter_finish), which the host and the device compile from one source;
 *             speechPlayer_pcmFilter executes them in a plain loop
 *   format 1  float32: out
 *   format 0  int16: the resampler's conversion of out (one float32 product by 32767, clipped to 32767 and -32768, rintf)
 *   filters   every coefficient is finite, and every section's poles lie strictly inside the unit circle, tested in binary64 on the
 *             float32 values: a2 < 1 and |a1| < 1 + a2; refused otherwise, the message naming the filter and the section
 * The bit-for-bit claim holds while every value stays finite; stable sections and |x| <= 2^16 keep it so for any sane filter.  A row some
 * value of which overflows is outside the claim: the device and the host may differ in the bits of its NaNs (nothing faults).
 * Lemma.  Appending or inserting an identity section (1 0 0 0 0) changes no output bit.  Its y = fmaf(1, x, s1) with s1 a zero equals x
 * except possibly in the sign of a zero; its states stay zeros (0 x, -0 y and their sums are zeros while x is finite); the sign of a zero
 * never changes a nonzero result downstream (a product with a zero is a zero, a zero added to a nonzero value returns it), so two such
 * runs agree everywhere except possibly in the signs of zeros; and the closing + 0.0f makes a zero +0.  This is what lets a wavefront pad
 * rows with fewer sections up to its instantiation's 1, 2, 4, 8 or 16.
 * Over the pool the result is a function of the batch's PCM: it depends on the mode and needs a synthesis launch.
 * Out of scope: live handles and initial conditions in or out through this export (the filter state would have to persist across pulls:
 * "Signal stages", below, keep it -- speechPlayer_batch_stageFilter); NodePlayer; zero-phase (forward-backward) filtering; time-parallel (scan) formulations, which cannot meet the sequential statement's bits.  For
 * the same reason a row cannot be cut in time: a call of fewer than 64 x 1024 rows underfills the device, and that is accepted.
 *
 * Host only, touch no device: the definition above on `length` samples of plain PCM (speechPlayer_pcmFilter) or of a signal's row,
 * int16 (inFormat 0) or float32 (inFormat 1) (speechPlayer_signalFilter), and one filter of nSections sections, sections being
 * float[nSections][5] -- the statements the device is held to bit for bit.  out: float[Lout] (format 1) or int16[Lout] (format 0).
 * Return Lout; a NULL out only sizes; -1 on tail outside 0 .. 2^20, a NULL sections, nSections outside 1 .. 16, a coefficient that is not
 * finite, a section whose poles are not strictly inside the unit circle, an unknown format or inFormat, length < 0 or above 2^44, a NULL
 * input with length > 0, a capacity below Lout, and (signalFilter) a float32 sample that is not finite or above 2^16 in magnitude. */
long long speechPlayer_pcmFilter(const sample* pcm, long long length, const float* sections, long long nSections, long long tail, int format, void* out,
	long long capacity);
long long speechPlayer_signalFilter(const void* x, int inFormat, long long length, const float* sections, long long nSections, long long tail, int format,
	void* out, long long capacity);
/* The chosen utterances' PCM (exportFiltered) or chosen rows of `signal` (exportFilteredOf), row i through filter filterOf[i], into
 * caller-owned device memory on the caller's stream.  The nFilters filters lie back to back in HOST memory: filter j is the sections
 * secStart[j] .. secStart[j+1]-1 of sections[][5] (filterOf NULL: nFilters must be 1).  filterOf is per ROW: with repeats in `utterances`
 * one utterance goes through several filters in one call.  utterances / rows, the rows' forms (rowStride > 0: padded rows, +0 past each
 * row's Lout; 0: the rows back to back), the return value, the device-memory checks, the sixteen-in-flight rule and the ordering by events
 * are those of speechPlayer_batch_exportConvolved / exportConvolvedOf.  The filters cross the link with the call's staging block and are
 * not kept on the batch (no new ordering state).  A wavefront takes 64 rows, a lane each, in tiles of kFilterTile = 64 samples
 * (csrc/klatt_filter.h); the rows are packed into wavefronts by instantiation and length, and the output order is the caller's.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what speechPlayer_batch_exportConvolved / exportConvolvedOf refuse of the
 * batch, the signal, the selection, the format, rowStride and the output; tail outside 0 .. 2^20; nFilters < 1; a NULL sections or
 * secStart; secStart not starting at 0; a filter of fewer than 1 or more than 16 sections; more than 2^16 sections in all; a
 * filterOf[i] outside 0 .. nFilters-1; filterOf NULL with nFilters != 1; a coefficient that is not finite and a section whose poles are
 * not strictly inside the unit circle (the message gives filter and section). */
long long speechPlayer_batch_exportFiltered(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const float* sections,
	const long long* secStart, long long nFilters, const long long* filterOf, long long tail, void* deviceOut, int format, long long rowStride,
	void* stream);
long long speechPlayer_batch_exportFilteredOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	const float* sections, const long long* secStart, long long nFilters, const long long* filterOf, long long tail, void* deviceOut, int format,
	long long rowStride, void* stream);
/*
 * A batch's PCM, or a signal's rows, through a speech codec: G.711 mu-law, G.711 A-law and IMA/DVI ADPCM -- what a telephone trunk or an ADPCM
 * handset does to a signal beyond band-limiting it, and (the 8-bit mu-law code) the class label per sample that autoregressive vocoders
 * train on.  codec: 0 "ulaw", 1 "alaw", 2 "adpcm".
 *   input     every codec takes an int16 sample s: a row's int16 itself; a float32 x through the resampler's conversion (one float32
 *             product by 32767, clipped to 32767 and -32768, rintf).  That conversion returns s for (float)s / 32767.0f, for all 65 536
 *             values of s, so an int16 row and its float32 form give the same outputs
 *   outputs   per sample, from one pass, either or both: the CODE, a uint8, ONE PER SAMPLE (0 .. 255 for G.711, 0 .. 15 for ADPCM: the rows
 *             stay on the grid of every other export; packing nibbles is the caller's, codes[0::2] << 4 | codes[1::2] being the usual byte
 *             order), and the DECODED sample d, what a decoder makes of the code: format 0 int16 d, format 1 float32 (float)d / 32767.0f.
 *             Row lengths are unchanged; there is no tail
 * All arithmetic is int32, >> is arithmetic, top(v) is the bit index of v's highest set bit.
 *   mu-law    encode  v = s >> 2; if v < 0 { v = -v; m = 0x7F } else m = 0xFF; if v > 8158: v = 8158; v += 33; seg = top(v) - 5;
 *                     code = ((seg << 4) | ((v >> (seg + 1)) & 15)) ^ m
 *                     (v stays below 8192 and seg within 0 .. 7; audioop clips at 8159 and answers the one sum that then reaches 8192
 *                     with the top code, which is the same code)
 *             decode  c = ~code & 255; t = (((c & 15) << 3) + 132) << ((c & 0x70) >> 4); d = (c & 0x80) ? 132 - t : t - 132
 *   A-law     encode  v = s >> 3; if v >= 0 m = 0xD5 else { m = 0x55; v = -v - 1 }; seg = v < 32 ? 0 : top(v) - 4;
 *                     code = ((seg << 4) | (seg < 2 ? (v >> 1) & 15 : (v >> seg) & 15)) ^ m
 *             decode  c = code ^ 0x55; t = (c & 15) << 4; seg = (c & 0x70) >> 4; seg 0: t += 8; seg 1: t += 0x108; else
 *                     t = (t + 0x108) << (seg - 1); d = (c & 0x80) ? t : -t
 *   ADPCM     the state val = 0, idx = 0 at a row's first sample; for each sample s, ascending:
 *                 step = STEP[idx]; diff = s - val; sign = diff < 0 ? 8 : 0; if sign: diff = -diff
 *                 delta = 0; vp = step >> 3
 *                 if diff >= step      { delta  = 4; diff -= step;      vp += step }
 *                 if diff >= step >> 1 { delta |= 2; diff -= step >> 1; vp += step >> 1 }
 *                 if diff >= step >> 2 { delta |= 1;                    vp += step >> 2 }
 *                 val = clamp(sign ? val - vp : val + vp, -32768, 32767)
 *                 code = delta | sign; idx = clamp(idx + INDEX[delta], 0, 88); d = val
 *             INDEX is -1 -1 -1 -1 2 4 6 8 and STEP the 89-entry IMA table (7 8 9 10 11 12 13 14 16 17 ... 27086 29794 32767:
 *             csrc/klatt_codec.h, kAdpcmTable).  A decoder given the codes rebuilds the same val -- vp is a function of step and code --,
 *             which is why d needs no second pass
 * The definition is the function bodies of csrc/klatt_codec.h, which the host and the device compile from one source; the G.711 laws and
 * the ADPCM recursion are those of CPython's audioop (tests/golden/codec_golden.npz records its answers).
 * Over the pool the result is a function of the batch's PCM: it depends on the mode and needs a synthesis launch.
 * Out of scope: G.722, G.726, GSM and anything without an independent statement to hold it to; packed nibbles and WAV block headers or
 * predictor resets; packet loss; live handles through this export (the ADPCM state would have to persist across pulls: "Signal stages",
 * below, keep it -- speechPlayer_batch_stageCode); NodePlayer.
 *
 * Host only, touch no device: the definition above on `length` samples of plain PCM (speechPlayer_pcmCode) or of a signal's row, int16
 * (inFormat 0) or float32 (inFormat 1) (speechPlayer_signalCode) -- the statements the device is held to bit for bit.  decodedOut:
 * float[length] (format 1) or int16[length] (format 0); codesOut: unsigned char[length]; either may be NULL, with length > 0 not both.
 * capacity: the elements each output given holds.  state (may be NULL): int[2], the ADPCM encoder's val and idx behind the last sample
 * (0 0 for a G.711 law).  Return length; -1 on an unknown inFormat, length < 0 or above 2^44, a NULL input with length > 0, an unknown
 * codec or format, no output, a capacity below length, and (signalCode) a float32 sample that is not finite or above 2^16 in magnitude. */
long long speechPlayer_pcmCode(const sample* pcm, long long length, int codec, int format, void* decodedOut, unsigned char* codesOut, long long capacity,
	int* state);
long long speechPlayer_signalCode(const void* x, int inFormat, long long length, int codec, int format, void* decodedOut, unsigned char* codesOut,
	long long capacity, int* state);
/* Host only: the decoder alone, `length` codes to `length` samples in `format`; for ADPCM the recursion above driven by the codes (state as
 * above: the decoder's).  Return length; -1 on length < 0 or above 2^44, NULL codes or a NULL out with length > 0, an unknown codec or
 * format, a capacity below length, and an ADPCM code above 15 (the message gives the code). */
long long speechPlayer_codecDecode(const unsigned char* codes, long long length, int codec, int format, void* out, long long capacity, int* state);
/* The chosen utterances' PCM (exportCoded) or chosen rows of `signal` (exportCodedOf) through `codec`, into caller-owned device memory on the
 * caller's stream: the decoded samples to decodedOut (format 0 int16, 1 float32), the codes to codesOut (unsigned char), either NULL but
 * not both; the same rowStride, in elements, lays out both.  utterances / rows, the rows' forms (rowStride > 0: padded rows, +0 and code 0
 * past each row's end; 0: the rows back to back), the return value (the elements of ONE output), the device-memory checks -- of each output
 * given --, the sixteen-in-flight rule and the ordering by events are those of speechPlayer_batch_exportFiltered / exportFilteredOf.
 * Nothing is kept on the batch.  A G.711 law runs tile-wise, a 256-lane workgroup per kCodeTile = 1024 samples of a row; ADPCM a wavefront
 * per 64 rows, a lane each, in tiles of kFilterTile = 64 samples (csrc/klatt_codec.h), the output order being the caller's.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: an unknown codec; both outputs NULL; what speechPlayer_batch_exportFiltered /
 * exportFilteredOf refuse of the format, rowStride, the batch, the signal, the selection and each output; outputs that overlap. */
long long speechPlayer_batch_exportCoded(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int codec, void* decodedOut,
	int format, unsigned char* codesOut, long long rowStride, void* stream);
long long speechPlayer_batch_exportCodedOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int codec, void* decodedOut, int format, unsigned char* codesOut, long long rowStride, void* stream);
/*
 * Signal stages: the resampler, the biquad filter and the codecs fed chunk by chunk -- what a live handle's pulls need.  The whole-row
 * exports above start every call from a fresh state, so calling them per pull clicks at every chunk edge and starts the ADPCM predictor
 * anew.  A STAGE is a device-resident object of a fixed number of rows that holds the per-row state of ONE sequential export between
 * calls.  It belongs to a batch, which gives it the device, the staging blocks and the sixteen-in-flight slots, as it does to the exports
 * of a signal: a batch that was never set is enough.  (The resampler's table is the stage's own, uploaded once when it is made: the
 * batch's table follows the last whole-row request.)  It is freed by speechPlayer_stage_free or with its batch.
 *   resample  (srcRate, outRate, zeros, rolloff, window, beta: the resampler's arguments and refusals.)  Per row: N, the samples
 *             consumed; M, the outputs emitted; and the last taps - 1 = 2 Z - 1 consumed samples as float32 -- x of what came in, +0
 *             before the start.  Equal rates pass the samples through and keep no state (Z = 0 below).
 *   filter    (sections, secStart, nFilters, filterOf, tail: the filter's arguments and refusals; filterOf is per row of the STAGE.)
 *             Per row: s1, s2 of each of its K sections.
 *   code      (codec 0 ulaw, 1 alaw, 2 adpcm.)  Per row: ADPCM's val and idx.  The G.711 laws carry none and take the same interface.
 * A PUSH takes a speechPlayer_signal_t of exactly nRows rows; row i of the signal is row i of the stage.  The rows are int16 or float32,
 * padded or packed, and the format may differ from push to push.  A row of length 0 is untouched.  end (may be NULL: none): per row,
 * nonzero ends the row with this push.  With c the row's length in this push and N' = N + c:
 *   resample, open   emits the outputs m = M .. M' - 1, M' = ceil(max(N' - Z, 0) up / down): exactly the outputs whose taps
 *                    n0 - Z + 1 .. n0 + Z, n0 = floor(m down / up), all lie at or before sample N' - 1 (n0 + Z <= N' - 1 <=> m down <
 *                    (N' - Z) up).  Inputs before sample 0 are +0, as in the definition.
 *   resample, ended  emits up to M' = ceil(N' up / down), the definition's count; inputs past N' - 1 are +0.  Afterwards the row is
 *                    fresh: N = M = 0, the history zeros.
 *   filter           open: c outputs, and the states as they are after exactly c samples.  Ended: c + tail outputs (tail samples of zero
 *                    input), then the states are +0.
 *   code             c outputs -- codes, decoded samples or both, as speechPlayer_batch_exportCoded --; ended: val = idx = 0 afterwards.
 * Lemma (the history's length).  With N consumed, output M is the first not emitted: n0(M) + Z > N - 1, so its oldest tap
 * n0(M) - Z + 1 >= N - 2 Z + 1, and n0 does not decrease with m: no later output reaches further back.  The samples N - 2 Z + 1 .. N - 1
 * are 2 Z - 1 values, which is what a row keeps.
 * The claim.  For every row, the outputs of its pushes up to and including the one that ends it, concatenated, are bit for bit what
 * speechPlayer_signalResample / speechPlayer_signalFilter (with tail) / speechPlayer_signalCode give on the concatenation of its chunks --
 * a chunk of int16 and a chunk of float32 count alike, each through x --, under those exports' bounds: finite samples of magnitude at
 * most 2^16, finite values in the filter.  A row pushed again after its end is a fresh row.
 * The outputs come as the exports' pair: deviceOut (format 0 int16, 1 float32; for a code stage the decoded samples) and, a code stage
 * only, deviceCodes (unsigned char), rowStride > 0 padded rows (+0 and code 0 past a row's outputs) or 0 the rows back to back;
 * outLengths (may be NULL): the nRows output counts.  They feed the next stage as its chunk.  Returns the elements of ONE output.
 * A push reads the chunk on `stream`, as the exports of a signal do; the pushes of one stage follow one another by events, whatever streams
 * they are issued on.  There are no repeats and no selection: a repeated row would race on its state.  A row's N may not pass 2^44.
 * speechPlayer_stage_plan is host only and changes nothing: what a push of rows of these lengths with these end flags would emit per row
 * (outLengths may be NULL); it returns their sum.  speechPlayer_stage_reset makes the chosen rows (rows[i] nonzero; NULL: all) fresh behind
 * the stage's last push; speechPlayer_stage_counts copies out N and M (either may be NULL).  speechPlayer_resampleEmitted is host only and
 * needs no stage: the outputs a resampler row has emitted after `consumed` samples, open or ended; the difference of two is a push's count.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT (the makers return NULL, the others -1), nothing written AND THE STATE UNCHANGED: what the
 * resampler, the filter and the codecs refuse of their arguments (when the stage is made); nRows outside 1 .. 2^20; a chunk whose row
 * count is not the stage's; what the exports of a signal refuse of the signal, the output, rowStride and the format; an output or
 * deviceCodes that overlaps the chunk, or the two each other; a row that would pass 2^44; a stage that was freed, alone or with its
 * batch (the handle names nothing any more); for a code stage, neither output given; deviceCodes on a stage that is not a code stage.
 * Out of scope in this section: the convolution, spectrogram, LPC, pitch and tempo exports chunk by chunk; saving a stage's state to the
 * host; NodePlayer; a fused kernel for a chain of stages ("Signal stages that keep a window", below, adds the convolution and the
 * spectrogram: speechPlayer_batch_stageConvolve, speechPlayer_batch_stageSpectrogram; "Signal stages on the step grid", behind it, adds LPC
 * and the pitch: speechPlayer_batch_stageLpc, speechPlayer_batch_stagePitch; tempo has no stage).  The kernels are csrc/klatt_stage.h.
 */
typedef void* speechPlayer_stage_t;
speechPlayer_stage_t speechPlayer_batch_stageResample(speechPlayer_batch_t batch, long long nRows, int srcRate, int outRate, int zeros, double rolloff,
	int window, double beta);
speechPlayer_stage_t speechPlayer_batch_stageFilter(speechPlayer_batch_t batch, long long nRows, const float* sections, const long long* secStart,
	long long nFilters, const long long* filterOf, long long tail);
speechPlayer_stage_t speechPlayer_batch_stageCode(speechPlayer_batch_t batch, long long nRows, int codec);
long long speechPlayer_stage_plan(speechPlayer_stage_t stage, const long long* lengths, const unsigned char* end, long long* outLengths);
long long speechPlayer_stage_push(speechPlayer_stage_t stage, const speechPlayer_signal_t* chunk, const unsigned char* end, void* deviceOut, int format,
	void* deviceCodes, long long rowStride, long long* outLengths, void* stream);
int speechPlayer_stage_reset(speechPlayer_stage_t stage, const unsigned char* rows, void* stream);
int speechPlayer_stage_counts(speechPlayer_stage_t stage, long long* consumed, long long* emitted);
void speechPlayer_stage_free(speechPlayer_stage_t stage);
long long speechPlayer_resampleEmitted(long long consumed, int srcRate, int outRate, int zeros, double rolloff, int ended);
/*
 * Signal stages that keep a window: the convolution and the spectrogram fed chunk by chunk -- the two ends of a live chain, the speech
 * through a room, a channel or a microphone first and the log-mel of what comes out last.  Both are stages as above (made on a batch, pushed
 * with speechPlayer_stage_push, planned, reset, counted and freed by the same entry points) whose per-row state is a window of the row's
 * most recent samples, float32 as x gave them and +0 before sample 0: the resampler stage's history with a length per row.
 * As above, a row has consumed N samples and emitted M outputs since its start; a push of c samples makes N' = N + c; an ended row is
 * fresh afterwards (N = M = 0, the history +0), and so is a row that speechPlayer_stage_reset names.
 *   convolution  (ir, irStart, nIr, irOf, tail: speechPlayer_batch_exportConvolved's arguments and refusals; irOf is per row of the
 *                STAGE.)  Row r has K_r taps and keeps H_r = K_r - 1 samples.  Open, a push emits c outputs, y[N .. N' - 1] of the row's
 *                stream.  Ended with tail 1: c + K_r - 1 outputs; ended with tail 0: c.
 *   spectrogram  (nFft, hop, phase, window, bank, nBands, power, logScale, floor: speechPlayer_batch_exportSpectrogram's arguments and
 *                refusals.)  Step j is centred on c_j = phase + j hop and reads the samples c_j - nFft / 2 .. c_j + nFft / 2 - 1: a frame
 *                (before, after) = (nFft / 2, nFft / 2 - 1).  Open, the steps emitted after N samples are those whose whole frame lies at
 *                or before sample N - 1: E_open(N) = 0 if N - after - 1 - phase < 0, else floor((N - after - 1 - phase) / hop) + 1.
 *                Ended: the definition's ceil((N - phase) / hop), 0 when N <= phase; samples past the end are +0, as the definition has
 *                them.  A push emits E(N', ended) - M steps.  A row keeps H = before + after = nFft - 1 samples.
 * Lemma (the convolution's bits).  speechPlayer_batch_exportConvolved's lemma applies: inserting or removing products that are +-0 changes
 * nothing behind the closing + 0.0f.  So the outputs H .. H + c - 1 (and the tail's) of the convolution of the virtual row
 * [history | chunk | +0] are the definition's, whether the history holds real samples or the +0 of a fresh row, and tap blocks whose
 * inputs all lie before the stream's first sample or past its last are skipped as the export skips them.
 * Lemma (the spectrogram's history).  Step M, the first not yet emitted with N consumed, has c_M > N - 1 - after, so its oldest sample
 * c_M - before >= N - (before + after); later steps reach no further back.  H = before + after = nFft - 1 samples therefore suffice
 * whatever hop and phase are, a hop above nFft (which skips samples) included.  Everything is in 64-bit integers; N <= 2^44, and a
 * hop or a phase above 2^45 means 2^45 (no row has that many samples).
 * The claim.  For every row, the outputs of its pushes up to and including the one that ends it, concatenated, are
 * speechPlayer_signalConvolve (with tail) / speechPlayer_signalSpectrogram of the concatenation of its chunks -- a chunk of int16 and a
 * chunk of float32 count alike, each through x --, under those exports' bounds: BIT FOR BIT for the convolution and for the spectrogram's
 * linear values; through the logarithm each side calls its own log10, and the device lies within 4 ulp of the host in float64, within one
 * float32 ulp of the rounded host value in float32.
 * The convolution's output is the other stages': deviceOut in format 0 int16 or 1 float32, rowStride > 0 padded rows (+0 past a row's
 * outputs) or 0 the rows back to back, outLengths the counts, so it feeds the next stage as its chunk.  The spectrogram's is
 * [row][step][bands] -- the bins nFft / 2 + 1 without a bank --: format 0 is float64 and 1 float32 (the spectrogram export's meanings, not
 * int16 / float32), rowStride is in STEPS (0: packed), outLengths are steps per row and the return value is the element count, steps times
 * bands; padding is +0.  It is not a signal, so a spectrogram stage ends a chain.  Window, twiddles, bank weights and ranges, and the
 * responses, are the stage's own, uploaded once when it is made.
 * speechPlayer_spectrogramEmitted is host only and needs no stage: the steps a spectrogram row has emitted after `consumed` samples, open
 * or ended; the difference of two is a push's count.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT (the makers return NULL, the others -1), nothing written AND THE STATE UNCHANGED: what the
 * whole-row exports refuse of the same arguments; nRows outside 1 .. 2^20; a stage whose histories -- the sum over its rows of H_r --
 * exceed 2^27 float32 per buffer (512 MiB; there are two), before anything is allocated; and of a push what the stages above refuse,
 * deviceCodes included.  speechPlayer_spectrogramEmitted refuses consumed outside 0 .. 2^44, an nFft that is no power of two in
 * 64 .. 4096, hop <= 0 and phase < 0.
 * Out of scope: LPC, pitch and tempo chunk by chunk are not in this section (the frame bookkeeping here is written for a general
 * (before, after) and serves the first two, which follow in "Signal stages on the step grid", below; tempo has no stage); a mix stage (an
 * SNR needs the whole row's power); FFT or MFMA convolution; saving a stage's state to the host; NodePlayer; a fused kernel for a chain.
 * The kernels are csrc/klatt_stage_window.h.
 */
speechPlayer_stage_t speechPlayer_batch_stageConvolve(speechPlayer_batch_t batch, long long nRows, const float* ir, const long long* irStart, long long nIr,
	const long long* irOf, int tail);
speechPlayer_stage_t speechPlayer_batch_stageSpectrogram(speechPlayer_batch_t batch, long long nRows, int nFft, long long hop, long long phase,
	const double* window, const double* bank, int nBands, int power, double logScale, double floor);
long long speechPlayer_spectrogramEmitted(long long consumed, int nFft, long long hop, long long phase, int ended);
/*
 * Signal stages on the step grid: the linear-prediction analysis and the pitch (YIN) fed chunk by chunk -- the frame features a live stream
 * needs beside its mu-law code (LPCNet-style vocoders), and the pitch a streaming front end tracks.  Both are stages as above (made on a
 * batch, pushed with speechPlayer_stage_push, planned, reset, counted and freed by the same entry points) whose per-row state is the
 * spectrogram stage's: a window of the row's most recent samples, float32 as x gave them and +0 before sample 0, H = before + after
 * samples of the frame (before, after) around a step's centre c_j = phase + j hop.
 *   LPC     (order, nWin, hop, phase, window, lagWindow, what: speechPlayer_batch_exportLpc's arguments and refusals.)  Step j reads the
 *           samples c_j - floor(nWin / 2) .. c_j - floor(nWin / 2) + nWin - 1, as the definition below has them: a frame (before, after)
 *           = (floor(nWin / 2), nWin - 1 - floor(nWin / 2)).  A row keeps H = nWin - 1 samples.  nCols = the values per step of `what`.
 *   pitch   (sampleRate, nWin = W, lagMin, lagMax, threshold, hop, phase, what: speechPlayer_batch_exportPitchOf's arguments and
 *           refusals.)  The frame has Nf = W + lagMax samples from c_j - floor(Nf / 2): (before, after) = (floor(Nf / 2), Nf - 1 -
 *           floor(Nf / 2)).  A row keeps H = Nf - 1 samples.  nCols = the values per step of `what`, lagMax - lagMin + 1 of them the CMND's.
 * The counts are the spectrogram stage's, with these (before, after): open, a row has emitted the steps whose whole frame lies at or before
 * sample N - 1, E_open(N) = 0 if N - after - 1 - phase < 0, else floor((N - after - 1 - phase) / hop) + 1; ended, the definition's
 * ceil((N - phase) / hop), 0 when N <= phase, samples past the end being +0.  A push emits E(N', ended) - M steps.  That H = before + after
 * samples suffice whatever hop and phase are is the lemma on the spectrogram's history above, which is stated for a general
 * (before, after).  A hop or a phase above 2^45 means 2^45; the sum of H over the rows is held to 2^27 float32 per buffer before anything
 * is allocated.
 * The output is laid out as the spectrogram stage's, [row][step][nCols]: format 0 is float64 and 1 float32, rowStride is in STEPS (0:
 * packed), outLengths are steps per row, the return value is steps times nCols, padding is +0, deviceCodes is refused.  Neither output is
 * a signal, so either stage ends a chain.  The window (float32) and the lag window (binary64) are the stage's own, uploaded once when it
 * is made.
 * The claim.  For every row, the outputs of its pushes up to and including the one that ends it, concatenated, are BIT FOR BIT
 * speechPlayer_signalLpc / speechPlayer_signalPitch of the concatenation of its chunks -- a chunk of int16 and a chunk of float32 count
 * alike, each through x --, under those exports' bounds.  There is no logarithm here and so no ulp bar: every field is bit-equal.  A row
 * pushed after its end or its reset is a fresh row.
 * speechPlayer_lpcEmitted and speechPlayer_pitchEmitted are host only and need no stage: the steps a row has emitted after `consumed`
 * samples, open or ended; the difference of two is a push's count.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT (the makers return NULL, the others -1), nothing written AND THE STATE UNCHANGED: what the
 * whole-row exports refuse of the same arguments; nRows outside 1 .. 2^20; histories beyond 2^27 samples in all; and of a push what the
 * spectrogram stage refuses.  The two *Emitted functions refuse consumed outside 0 .. 2^44, hop <= 0, phase < 0, an nWin outside 2 .. 4096
 * (LPC) or 32 .. 2048 (pitch) and a lagMax outside 3 .. 1024.
 * Out of scope: the residual or the prediction (speechPlayer_batch_exportLpcResidual) chunk by chunk -- a sample's frame is the nearest
 * centre, so it needs frames still to come --; tempo; a mix stage; saving a stage's state to the host; NodePlayer; a fused kernel for a
 * chain.  The kernels are csrc/klatt_stage_frames.h.
 */
speechPlayer_stage_t speechPlayer_batch_stageLpc(speechPlayer_batch_t batch, long long nRows, int order, int nWin, long long hop, long long phase,
	const double* window, const double* lagWindow, int what);
speechPlayer_stage_t speechPlayer_batch_stagePitch(speechPlayer_batch_t batch, long long nRows, int sampleRate, int nWin, int lagMin, int lagMax,
	double threshold, long long hop, long long phase, int what);
long long speechPlayer_lpcEmitted(long long consumed, int nWin, long long hop, long long phase, int ended);
long long speechPlayer_pitchEmitted(long long consumed, int nWin, int lagMax, long long hop, long long phase, int ended);
/*
 * Linear prediction (LPC) of a batch's PCM, or of a signal's rows, on the step grid of the other exports: per analysis frame the
 * autocorrelation, the prediction coefficients, the reflection coefficients and the prediction error; and, per sample, the residual or
 * the prediction by the frames' own coefficients -- what autoregressive vocoders of the LPCNet family and every classical speech front
 * end take beside the mu-law code, and the classical estimate of the vocal-tract envelope that speechPlayer_batch_exportResponse states
 * exactly.  A row of L samples is read as the other exports of the PCM read it: an int16 s is (float)s / 32767.0f, a float32 is taken as
 * it is, a sample outside 0 .. L-1 is +0 and nothing is loaded there.
 *   steps     the spectrogram's grid, row for row: step j is centred on c = phase + j * hop; a row has ceil((L - phase) / hop) steps, 0 when
 *             L <= phase
 *   frame     x[i] is sample c - floor(nWin / 2) + i for i = 0 .. nWin-1.  order lies in 1 .. 32 (kLpcMaxOrder); nWin is any integer with
 *             order < nWin <= 4096 (kLpcMaxWin), not only a power of two (20 to 25 ms windows are 320, 400, 551 samples)
 *   window    window[nWin], a HOST array of doubles, each rounded to float32 once; NULL: the periodic Hann 0.5 - 0.5 cos(2 pi i / nWin),
 *             evaluated in binary64 on the host.  xw[i] = x[i] * w[i], one float32 product
 *   autocorrelation   for k = 0 .. order: term(i, k) = (double)xw[i] * (double)xw[i - k], exact in binary64 (fusing it into an FMA changes
 *             no bit); partial[q], q = 0 .. 63, is the sum from +0.0, in ascending i, of term(i, k) over k <= i < nWin with i mod 64 == q;
 *             r[k] is the balanced binary tree over the 64 partials in natural order, t[i] = t[2i] + t[2i+1], six levels.  A partial that
 *             starts from +0.0 is never -0.0, and adding +-0 to a value that is not -0.0 changes no bit, so terms with a zero factor
 *             (samples outside the row, the exact zeros of a silence) may be skipped
 *   lag window   lagWindow[order + 1], a HOST array of finite doubles: r[k] <- r[k] * lagWindow[k], one binary64 product; NULL: no
 *             multiplication at all.  White-noise correction is lagWindow[0] = 1 + eps; Gaussian lag windowing the rest
 *   recursion (Levinson-Durbin), entirely in binary64 with explicit fma:
 *                 E = r[0]; a[1..order] = k[1..order] = +0.0; stages = 0
 *                 for i = 1 .. order:
 *                     if not (E > 0 and E finite): stop
 *                     acc = r[i];  for j = 1 .. i-1 ascending: acc = fma(a[j], r[i-j], acc)
 *                     kappa = -acc / E
 *                     if not (|kappa| < 1): stop          (a NaN stops too: the frame is not positive definite in binary64)
 *                     for j = 1 .. i-1: a'[j] = fma(kappa, a[i-j], a[j])   (all from the old a)
 *                     a = a'; a[i] = kappa; k[i] = kappa
 *                     E = fma(kappa, acc, E); stages = i
 *             Sign convention: A(z) = 1 + sum a_j z^-j; the prediction of x(t) is -sum a_j x(t-j).  A silent frame (r[0] = +0) gives
 *             stages = 0 and all values +0
 *   fields    `what` is a bit set; the fields come in this fixed order whatever the order of the bits: 1 AUTOCORR order + 1 values, r
 *             after the lag window; 2 LPC order values, a_1 .. a_order; 4 REFLECTION order values, k_1 .. k_order; 8 ERROR one value, E;
 *             16 STAGES one value, stages as a number.  nCols is their total
 *   output    element (row, step, col) of [row][step][nCols]; format 0 float64, 1 float32 rounded to nearest
 * The inverse filter: a row's samples through the time-varying FIR of its own frames' coefficients -- no recursion, no synthesis of its
 * own.  The coefficients come from a DEVICE tensor [row][step][coeffCols] (format 0 float64, 1 float32 widened exactly), a_1 .. a_order at
 * columns col0 .. col0 + order - 1: one the analysis wrote for the same rows, hop and phase, or the caller's own (bandwidth-expanded,
 * quantised, a network's).  coeffStride is in steps: 0 packed, else padded; row i of the tensor belongs to the i-th chosen row.
 *   frame of a sample   for sample t of a row with steps > 0: j = min(steps - 1, (max(t - phase, 0) + floor(hop / 2)) / hop) in 64-bit
 *             integers -- the nearest centre, ties upward.  A row without steps uses coefficients +0
 *   residual  (what 0) s = (double)x(t); for m = 1 .. order ascending: s = fma(a_m, (double)x(t - m), s); e(t) = (float)s
 *   prediction   (what 1) the same chain from +0.0; p(t) = (float)(-s)
 *   output    L samples per row; format 1 float32, format 0 int16 by the resampler's conversion of the float32 value; padded or packed as
 *             the resampled, filtered and coded exports are, so (tensor, lengths) is a signal for the next stage
 * Bits are unspecified for non-finite coefficients, as for samples outside the signal bound; no value ever steers an address.
 * The definition is the function bodies of csrc/klatt_lpc.h, which the host and the device compile from one source.  Over the pool the
 * result is a function of the batch's PCM: it depends on the mode and needs a synthesis launch.
 * Out of scope: line spectral frequencies; Burg and covariance methods; the recursive synthesis filter 1 / A(z) inside these exports (it is
 * an export of its own: "LPC synthesis", below); order above 32;
 * pre-emphasis inside the export (the chain is exportFiltered with a pre-emphasis section, then the signal form); live handles through
 * this export (the last nWin - 1 samples would have to persist across pulls: "Signal stages on the step grid", above, keep them for the
 * analysis -- speechPlayer_batch_stageLpc; the residual has no stage); NodePlayer beyond speechPlayer_node_part.
 *
 * Host only, touches no device: the recursion alone on r[order + 1].  a and k take order values each (a_1 .., k_1 ..), error E, stages the
 * stages done; each may be NULL.  Returns order; -1 on order outside 1 .. 32 or a NULL r. */
long long speechPlayer_lpcFromAutocorrelation(const double* r, int order, double* a, double* k, double* error, int* stages);
/* Host only, touch no device: the analysis above on `length` samples of plain PCM (speechPlayer_pcmLpc) or of a signal's row, int16
 * (inFormat 0) or float32 (inFormat 1) (speechPlayer_signalLpc), out[step][nCols] float64 -- the statements the device is held to bit for
 * bit.  Return steps * nCols; -1 on an unknown inFormat, length < 0 or above 2^44, a NULL input with length > 0, hop <= 0, phase < 0,
 * order outside 1 .. 32, nWin outside order + 1 .. 4096, a non-finite window or lagWindow value, what 0 or with a bit above 16, a NULL out
 * with steps > 0, and (signalLpc) a float32 sample that is not finite or above 2^16 in magnitude. */
long long speechPlayer_pcmLpc(const sample* pcm, long long length, int order, int nWin, long long hop, long long phase, const double* window,
	const double* lagWindow, int what, double* out);
long long speechPlayer_signalLpc(const void* x, int inFormat, long long length, int order, int nWin, long long hop, long long phase,
	const double* window, const double* lagWindow, int what, double* out);
/* Host only: the inverse filter above on `length` samples with the coefficients a HOST array double[steps][order]; out float[length]
 * (format 1) or int16[length] (format 0) of `capacity` elements.  Return length; -1 on an unknown inFormat, length < 0 or above 2^44, a
 * NULL input with length > 0, hop <= 0, phase < 0, order outside 1 .. 32, what outside {0, 1}, an unknown format, NULL coefficients with
 * steps > 0, a NULL out with length > 0, a capacity below length, and (signalLpcResidual) a float32 sample outside the signal bound. */
long long speechPlayer_pcmLpcResidual(const sample* pcm, long long length, int order, long long hop, long long phase, const double* coeff, int what,
	int format, void* out, long long capacity);
long long speechPlayer_signalLpcResidual(const void* x, int inFormat, long long length, int order, long long hop, long long phase, const double* coeff,
	int what, int format, void* out, long long capacity);
/* The analysis of chosen utterances (exportLpc) or of chosen rows of `signal` (exportLpcOf) into caller-owned device memory on the caller's
 * stream.  utterances / rows (any order, repeats allowed, NULL: all), rowStride (in steps, +0 past a row's end; 0: the rows back to back),
 * the return value (elements written; 0 writes nothing and needs no buffer), the ordering by events, the sixteen-in-flight rule, the
 * device-memory, alignment and size checks and the signal contract (not the pool, no synthesis needed, the output may not overlap the
 * signal) are those of speechPlayer_batch_exportSpectrogram / exportSpectrogramOf.  A 256-lane workgroup takes 64 consecutive steps of the
 * output (csrc/klatt_lpc.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what speechPlayer_batch_exportSpectrogram / exportSpectrogramOf refuse of the
 * batch, the signal, hop, phase, the format, the selection, rowStride and the output; order outside 1 .. 32; nWin outside order + 1 ..
 * 4096; a non-finite window or lagWindow value; what 0 or with a bit above 16. */
long long speechPlayer_batch_exportLpc(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, int nWin,
	long long hop, long long phase, const double* window, const double* lagWindow, int what, void* deviceOut, int format, long long rowStride,
	void* stream);
long long speechPlayer_batch_exportLpcOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int order, int nWin, long long hop, long long phase, const double* window, const double* lagWindow, int what, void* deviceOut, int format,
	long long rowStride, void* stream);
/* The residual (what 0) or the prediction (what 1) of chosen utterances (exportLpcResidual) or of chosen rows of `signal`
 * (exportLpcResidualOf), the coefficients read from deviceCoeff as described above.  utterances / rows, the rows' forms (rowStride in
 * samples), the return value, the device-memory checks, the sixteen-in-flight rule and the ordering by events are those of
 * speechPlayer_batch_exportFiltered / exportFilteredOf; the caller orders whatever wrote the coefficients before the export on `stream`.
 * Tile-wise, a 256-lane workgroup per kLpcTile = 1024 samples of a row (csrc/klatt_lpc.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what speechPlayer_batch_exportFiltered / exportFilteredOf refuse of the
 * format, rowStride, the batch, the signal, the selection and the output; order outside 1 .. 32; hop <= 0; phase < 0; what outside
 * {0, 1}; an unknown coeffFormat; col0 < 0 or col0 + order > coeffCols; a coeffStride below the largest step count; a coefficient tensor
 * that is not device memory of the batch's device, misaligned to its element or too small for the rows' steps; an output that overlaps the
 * coefficients or the signal. */
long long speechPlayer_batch_exportLpcResidual(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, long long hop,
	long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride, int what, void* deviceOut, int format,
	long long rowStride, void* stream);
long long speechPlayer_batch_exportLpcResidualOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int order, long long hop, long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride, int what,
	void* deviceOut, int format, long long rowStride, void* stream);
/*
 * LPC synthesis: a row of excitation samples through the recursive all-pole filter 1 / A(z) of its frames' prediction coefficients -- the
 * inverse of the inverse filter above, and the decoder half of what the other two exports give: analysis-synthesis with changed
 * coefficients (bandwidth expansion, quantised reflection coefficients, another speaker's envelope), cross-synthesis, x = e + p where e is
 * not the exact residual.  A row of L excitation samples e(0 .. L-1) is read as the other exports read a row: an int16 s is
 * (float)s / 32767.0f, a float32 is taken as it is; the row is the pool's utterance or a signal's row.  The coefficients come from a
 * DEVICE tensor [row][step][coeffCols] (format 0 float64, 1 float32 widened exactly), a_1 .. a_order at columns col0 .. col0 + order - 1,
 * coeffStride in steps (0 packed, else padded), row i of the tensor belonging to the i-th chosen row: exactly as
 * speechPlayer_batch_exportLpcResidual reads them, for the same hop and phase.  order lies in 1 .. 32, one per call.
 *   frame of a sample   lpc_frame_of(t, hop, phase, steps): j = min(steps - 1, (max(t - phase, 0) + floor(hop / 2)) / hop), the nearest
 *             centre, ties upward.  A row without steps uses coefficients +0
 *   recursion y(t) = +0 for t < 0.  For t = 0 .. L-1 ascending: s = (double)e(t); for m = 1 .. order ascending:
 *             s = fma(-a_m, (double)y(t - m), s) -- the negation is exact, the fma explicit --; y(t) = (float)s
 *   history   the history is the float32 y, never the int16 of the output
 *   bounds    the loops run behind m <= order tests: no row is padded with zero coefficients, because fma(-0.0, y, s) can change the sign
 *             of a zero
 *   output    L samples per row; format 1 float32 y(t), format 0 int16 by the resampler's conversion of y(t); padded (rowStride, +0 past
 *             a row's end) or packed, so (tensor, lengths) is a signal for the next stage
 * Unstable coefficients cannot be refused, since they live on the device: once a value of a row is not finite, that row's later bits are
 * unspecified.  It faults nothing and no value steers an address.
 * The definition is the function bodies of csrc/klatt_lpcsynth.h, which the host and the device compile from one source: one wavefront per
 * 64 rows, a lane per row, the history a register ring of 8, 16 or 32 slots (the smallest >= order).
 * Out of scope: initial conditions in or out; a pole-zero or weighting filter A(z/g1)/A(z/g2); order above 32; a live stage (a stage takes
 * one input; this takes two); NodePlayer; time-parallel formulations (they cannot meet the sequential statement's bits).
 *
 * Host only, touch no device: the recursion above on `length` samples with the coefficients a HOST array double[steps][order]; out
 * float[length] (format 1) or int16[length] (format 0) of `capacity` elements.  Return length; -1 on an unknown inFormat, length < 0 or
 * above 2^44, a NULL input with length > 0, hop <= 0, phase < 0, order outside 1 .. 32, an unknown format, NULL coefficients with steps > 0,
 * a NULL out with length > 0, a capacity below length, and (signalLpcSynthesis) a float32 sample outside the signal bound. */
long long speechPlayer_pcmLpcSynthesis(const sample* pcm, long long length, int order, long long hop, long long phase, const double* coeff, int format,
	void* out, long long capacity);
long long speechPlayer_signalLpcSynthesis(const void* x, int inFormat, long long length, int order, long long hop, long long phase, const double* coeff,
	int format, void* out, long long capacity);
/* Host only, touches no device: a_1 .. a_order from the reflection coefficients k_1 .. k_order by the step-up recursion, which is exactly
 * the Levinson-Durbin recursion's update: for i = 1 .. order: a'[j] = fma(k_i, a[i-j], a[j]) for j = 1 .. i-1, all from the old a, then
 * a[i] = k_i.  |k_i| < 1 for every i gives a stable 1 / A(z): this is how a caller gets stable coefficients out of modified or quantised
 * reflection coefficients.  Returns order; -1 on order outside 1 .. 32 or a NULL argument. */
long long speechPlayer_lpcFromReflection(const double* k, int order, double* a);
/* The synthesis of chosen utterances (exportLpcSynthesis) or of chosen rows of `signal` (exportLpcSynthesisOf), the coefficients read from
 * deviceCoeff as described above.  The arguments are speechPlayer_batch_exportLpcResidual / exportLpcResidualOf's without `what`;
 * utterances / rows, the rows' forms (rowStride in samples), the return value, the device-memory, alignment and overlap checks, the
 * sixteen-in-flight rule and the ordering by events are theirs; the caller orders whatever wrote the coefficients before the export on
 * `stream`.  Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what they refuse, `what` apart. */
long long speechPlayer_batch_exportLpcSynthesis(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int order, long long hop,
	long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride, void* deviceOut, int format,
	long long rowStride, void* stream);
long long speechPlayer_batch_exportLpcSynthesisOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int order, long long hop, long long phase, const void* deviceCoeff, int coeffFormat, int coeffCols, int col0, long long coeffStride,
	void* deviceOut, int format, long long rowStride, void* stream);
/*
 * Pitch ESTIMATED FROM THE SIGNAL (YIN) of a batch's PCM, or of a signal's rows, on the step grid of the other exports: per analysis frame
 * the period, the fundamental, a periodicity measure and the voicing decision -- the one feature the LPCNet family and the classical front
 * ends take that the other exports plus a matrix product cannot give.  speechPlayer_batch_exportSource states the TRUE fundamental of the
 * clean synthesis; this export estimates it from a row that has been through a room, a noise mix, a codec or a tempo change, which is what a
 * front end sees.  A row of L samples is read as the other exports of the PCM read it: an int16 s is (float)s / 32767.0f, a float32 is taken
 * as it is, a sample outside 0 .. L-1 is +0 and nothing is loaded there.
 *   per call  nWin = W, any integer in 32 .. 2048 (kPitchMaxWin); 2 <= lagMin < lagMax <= 1024 (kPitchMaxLag); threshold a finite double in
 *             [0, 1]; hop > 0, phase >= 0; sampleRate > 0 serves the F0 field alone: the batch's own (exportPitch) or the argument
 *             (exportPitchOf and the host statements), as exportResampledOf takes srcRate
 *   steps     the spectrogram's grid, row for row: step j is centred on c = phase + j * hop; a row has ceil((L - phase) / hop) steps, 0 when
 *             L <= phase
 *   frame     N = W + lagMax; x[i] is sample c - floor(N / 2) + i for i = 0 .. N-1
 *   difference   for tau = 1 .. lagMax: u(i) = x[i] - x[i + tau], ONE binary32 subtraction; term(i) = (double)u * (double)u, exact in
 *             binary64; four chains c_j, j = i mod 4, each the sum from +0.0, in ascending i over 0 <= i < W, of its terms, one rounding an
 *             addition (an fma does it); d(tau) = (c_0 + c_1) + (c_2 + c_3).  A chain that starts from +0.0 is never -0.0, so terms with
 *             u == 0 may be skipped.  Inside the signal bound (finite, |x| <= 2^16) every value is finite
 *   cumulative mean   s(0) = +0.0; s(tau) = s(tau - 1) + d(tau) in ascending tau; m(tau) = s(tau) > 0 ? (d(tau) * (double)tau) / s(tau) : 1.0,
 *             one product and one division
 *   choice    tau* is the lowest tau in lagMin .. lagMax with m(tau) < threshold and (tau == lagMax or !(m(tau + 1) < m(tau))): voiced = 1.
 *             If there is none, voiced = 0 and tau* is the tau of the least m(tau) in the range, ties to the lowest tau.  Both rules are
 *             minima under a total order: only the choice crosses lanes
 *   refinement   if tau* - 1 >= 1 and tau* + 1 <= lagMax: with y0, y1, y2 = m at tau* - 1, tau*, tau* + 1, den = (y0 - y1) + (y2 - y1); if
 *             den > 0: delta = (0.5 * (y0 - y2)) / den, used only if fabs(delta) <= 0.5.  In every other case delta = +0.0.
 *             period = (double)tau* + delta
 *   fields    `what` is a bit set; the fields come in this fixed order whatever the order of the bits: 1 F0 voiced ? (double)sampleRate /
 *             period : +0.0; 2 PERIOD the period, always; 4 LAG tau* as a number; 8 APERIODICITY m(tau*); 16 VOICED 0 or 1; 32 CMND
 *             m(lagMin .. lagMax), lagMax - lagMin + 1 values, for a tracker of the caller's own (Viterbi, pYIN).  nCols is their total
 *   output    element (row, step, col) of [row][step][nCols]; format 0 float64, 1 float32 rounded once; +0 past a row's steps in the padded
 *             form
 * The definition is the function bodies of csrc/klatt_pitch.h, which the host and the device compile from one source.  Over the pool the
 * result is a function of the batch's PCM: it depends on the mode and needs a synthesis launch.
 * Known behaviour of the method: the first dip below the threshold may be a formant's, not the period's -- vowel i at 220 Hz and 22050 Hz has
 * m = 0.11 at lag 95 beside the period of 100.2 samples --; the CMND field exists so that a tracker can decide otherwise.
 * Out of scope: normalised cross-correlation and energies; smoothing or tracking across steps; octave-error correction; FFT or MFMA
 * evaluation of the difference (their summation order is not the definition's); decimation inside the export (the chain is
 * exportResampled to 16000 Hz, then the signal form); live handles through this export ("Signal stages on the step grid", above, keep the
 * last nWin + lagMax - 1 samples across pulls -- speechPlayer_batch_stagePitch); NodePlayer beyond speechPlayer_node_part.
 *
 * Host only, touch no device: the estimate above on `length` samples of plain PCM (speechPlayer_pcmPitch) or of a signal's row, int16
 * (inFormat 0) or float32 (inFormat 1) (speechPlayer_signalPitch), out[step][nCols] float64 -- the statements the device is held to bit for
 * bit.  Return steps * nCols; -1 on an unknown inFormat, length < 0 or above 2^44, a NULL input with length > 0, hop <= 0, phase < 0,
 * sampleRate <= 0, nWin outside 32 .. 2048, lagMin < 2, lagMin >= lagMax, lagMax > 1024, a threshold outside [0, 1] or not finite, what 0 or
 * with a bit above 32, a NULL out with steps > 0, and (signalPitch) a float32 sample that is not finite or above 2^16 in magnitude. */
long long speechPlayer_pcmPitch(const sample* pcm, long long length, int sampleRate, int nWin, int lagMin, int lagMax, double threshold,
	long long hop, long long phase, int what, double* out);
long long speechPlayer_signalPitch(const void* x, int inFormat, long long length, int sampleRate, int nWin, int lagMin, int lagMax,
	double threshold, long long hop, long long phase, int what, double* out);
/* The estimate of chosen utterances (exportPitch, at the batch's sample rate) or of chosen rows of `signal` (exportPitchOf, at sampleRate)
 * into caller-owned device memory on the caller's stream.  utterances / rows, rowStride (in steps; 0: packed), the return value, the ordering
 * by events, the sixteen-in-flight rule, the device-memory, alignment and size checks and the signal contract are those of
 * speechPlayer_batch_exportLpc / exportLpcOf.  A 256-lane workgroup takes 16 consecutive steps of the output, a wavefront a step at a time
 * (csrc/klatt_pitch.h).
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written, the batch still usable: what speechPlayer_batch_exportLpc / exportLpcOf refuse
 * of the batch, the signal, hop, phase, the format, the selection, rowStride and the output; nWin, lagMin, lagMax, threshold or sampleRate
 * out of the ranges above; what 0 or with a bit above 32. */
long long speechPlayer_batch_exportPitch(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int nWin, int lagMin,
	int lagMax, double threshold, long long hop, long long phase, int what, void* deviceOut, int format, long long rowStride, void* stream);
long long speechPlayer_batch_exportPitchOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	int sampleRate, int nWin, int lagMin, int lagMax, double threshold, long long hop, long long phase, int what, void* deviceOut, int format,
	long long rowStride, void* stream);
/*
 * Tempo perturbation of a batch's PCM, or of a signal's rows, by waveform-similarity overlap-add (WSOLA): the duration changes, the pitch
 * and the formants stay.  Beside the samples the export gives its time map, the input sample every output frame was taken from.  A row
 * of L samples is read as the other exports of the PCM read it: an int16 s is (float)s / 32767.0f, a float32 is taken as it is, a sample
 * outside 0 .. L-1 is +0 and nothing is loaded there.
 *   per call  nWin = N, even, 64 .. 2048 (kTempoMaxWin); Hs = N / 2.  search = D, 0 .. 1024 (kTempoMaxSearch)
 *   per OUTPUT row   tempo, a finite double in [0.25, 4]; a tempo above 1 gives a shorter output
 *   lengths   (host only) Lout = (long long)ceil((double)L / tempo), one binary64 division; Lout = 0 for L = 0.  K = ceil(Lout / Hs) + 1
 *             frames when Lout > 0, else 0
 *   window    w[i] is the float32 of 0.5 - 0.5 cos(2 pi i / N), i = 0 .. N-1, evaluated in binary64 on the host
 *   positions p[k], k = 0 .. K-1, 64-bit integers: p[k] is the input sample placed at output k * Hs; p[0] = 0.  For k >= 1:
 *             a = (long long)floor((double)(k * Hs) * tempo), one binary64 product; the template is T[i] = x(p[k-1] + i), the natural
 *             continuation of the previous segment; the candidate at lag d is C_d[i] = x(a - Hs + d + i), i = 0 .. N-1, d = -D .. D
 *   score     term(i) = (double)T[i] * (double)C_d[i], exact in binary64 (fusing it into an FMA changes no bit); four chains c_j,
 *             j = 0 .. 3, each the sum from +0.0, in ascending i, of term(i) over i mod 4 == j; score(d) = (c_0 + c_1) + (c_2 + c_3).  A
 *             chain that starts from +0.0 is never -0.0, so terms with a zero factor may be skipped
 *   choice    p[k] = a + d*, d* of the greatest score compared as binary64 values, ties to the lowest rank(d) = 2|d| - (d < 0 ? 1 : 0):
 *             0, -1, +1, -2, +2, ...  A silent or constant stretch therefore takes d = 0.  Inputs inside the signal bound (finite,
 *             magnitude at most 2^16) give finite scores; outside it the bits are unspecified
 *   render    for output m = 0 .. Lout-1: q = m / Hs, i = m - q * Hs,
 *                 y(m) = fmaf(w[Hs + i], x(P[q] + i), w[i] * x(P[q+1] - Hs + i)) + 0.0f
 *             each operation one correctly rounded binary32 operation; P[k] = min(max(p[k], -2^45), 2^45), so the positions may be the
 *             caller's own, of any value: a position steers an address only behind the row's mask, nothing outside the row is loaded
 *   output    Lout samples per row; format 1 float32, format 0 int16 by the resampler's conversion; padded or packed as the resampled
 *             export is, so (tensor, lengths) is a signal for the next stage
 * The definition is the function bodies of csrc/klatt_tempo.h, which the host and the device compile from one source.  Over the pool the
 * result is a function of the batch's PCM: it depends on the mode and needs a synthesis launch.
 * Limits      as the signal contract's (above); tests/test_gpu_tempo.py runs the render past elements 2^31 and 2^32 of its output.
 * Out of scope: normalised cross-correlation; custom windows or hops other than N / 2; phase-vocoder and PSOLA methods; pitch shifting (this
 * export followed by the resampler does it); warping the label grids on the device; live handles; NodePlayer beyond
 * speechPlayer_node_part; filling the chip with few rows (a row's frames are sequential, as a filter's samples are).
 *
 * Host only, touch no device: Lout and K of a row of `length` samples.  -1 on length < 0 or above 2^44, a tempo that is not finite or
 * outside [0.25, 4], and (tempoFrames) nWin odd or outside 64 .. 2048. */
long long speechPlayer_tempoLength(long long length, double tempo);
long long speechPlayer_tempoFrames(long long length, double tempo, int nWin);
/* Host only: the definition above on `length` samples of plain PCM (speechPlayer_pcmTempo) or of a signal's row, int16 (inFormat 0) or
 * float32 (inFormat 1) (speechPlayer_signalTempo) -- the statements the device is held to bit for bit.  positionsIn NULL: the search runs
 * and positionsOut (may be NULL) receives the K positions; else positionsIn[K] is rendered (search is not looked at) and copied to
 * positionsOut.  out is float[Lout] (format 1) or int16[Lout] (format 0) of `capacity` elements; a NULL out only sizes, and still fills
 * positionsOut.  Return Lout; -1 on an unknown inFormat, a NULL input with length > 0, the refusals of tempoLength, an unknown format,
 * nWin odd or outside 64 .. 2048, search outside 0 .. 1024, a capacity below Lout, and (signalTempo) a float32 sample that is not finite
 * or above 2^16 in magnitude. */
long long speechPlayer_pcmTempo(const sample* pcm, long long length, double tempo, int nWin, int search, const long long* positionsIn,
	long long* positionsOut, int format, void* out, long long capacity);
long long speechPlayer_signalTempo(const void* x, int inFormat, long long length, double tempo, int nWin, int search, const long long* positionsIn,
	long long* positionsOut, int format, void* out, long long capacity);
/* The positions of chosen utterances (exportTempoPositions) or of chosen rows of `signal` (exportTempoPositionsOf): int64 [row][K] into
 * caller-owned device memory on the caller's stream.  tempo is a HOST array, one double per OUTPUT row.  rowStride is in frames (0: the
 * rows back to back); past a row's K the value is 0.  utterances / rows (any order, repeats allowed -- one utterance at several tempos --,
 * NULL: all), the return value (elements written; 0 writes nothing and needs no buffer), the device-memory, alignment and overlap checks,
 * the ordering by events, the sixteen-in-flight rule and the signal contract are those of speechPlayer_batch_exportResampled /
 * exportResampledOf.  One 256-lane workgroup per row, rows longest first (csrc/klatt_tempo.h).  Nothing is kept on the batch.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what exportResampled / exportResampledOf refuse of the batch, the signal,
 * the selection, rowStride and the output; nWin odd or outside 64 .. 2048; search outside 0 .. 1024; a NULL tempo, or one that is not
 * finite or lies outside [0.25, 4] (the message names the row). */
long long speechPlayer_batch_exportTempoPositions(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const double* tempo,
	int nWin, int search, long long* devicePositions, long long rowStride, void* stream);
long long speechPlayer_batch_exportTempoPositionsOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	const double* tempo, int nWin, int search, long long* devicePositions, long long rowStride, void* stream);
/* The chosen rows rendered from devicePositions, a DEVICE tensor [row][K] of int64: what exportTempoPositions wrote for the same rows,
 * tempo and nWin, or the caller's own.  posStride is in frames: 0 packed, otherwise padded; row i of the tensor belongs to the i-th chosen
 * row.  Formats and rowStride (in samples) are speechPlayer_batch_exportResampled's, and so are the selection, the return value, the
 * checks of the output and the signal, the ordering by events and the sixteen-in-flight rule; the caller orders whatever wrote the
 * positions before the export on `stream`.  Tile-wise, a 256-lane workgroup per kTempoTile = 1024 outputs of a row.
 * Refused with SPEECHPLAYER_ERR_ARGUMENT and nothing written: what exportResampled / exportResampledOf refuse; nWin odd or outside
 * 64 .. 2048; a NULL tempo, or one that is not finite or lies outside [0.25, 4]; a posStride below the largest K; a positions tensor that
 * is not device memory of the batch's device, misaligned to 8 bytes or too small; an output that overlaps the positions or the signal. */
long long speechPlayer_batch_exportTempo(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, const double* tempo, int nWin,
	const long long* devicePositions, long long posStride, void* deviceOut, int format, long long rowStride, void* stream);
long long speechPlayer_batch_exportTempoOf(speechPlayer_batch_t batch, const speechPlayer_signal_t* signal, const long long* rows, long long nRows,
	const double* tempo, int nWin, const long long* devicePositions, long long posStride, void* deviceOut, int format, long long rowStride, void* stream);
/* The HIP device the batch is bound to (-1: no batch). */
int speechPlayer_batch_device(speechPlayer_batch_t batch);

/* The frames of utterance u as they are resident in HBM (downloaded; after any of the set calls): what each speechPlayer_queueFrame
 * call of that utterance would have been given.  Returns the utterance's number of frames; fills the arrays (each may be NULL)
 * when it is <= capacity.  fadeDuration comes back as the engine uses it (>= 1: reference src/speechPlayer.cpp:36). */
long long speechPlayer_batch_frames(speechPlayer_batch_t batch, long long utterance, speechPlayer_frame_t* frames,
	unsigned int* minFrameDuration, unsigned int* fadeDuration, int* userIndex, unsigned char* isNull, long long capacity);

/* Number of samples utterance u produces: sum over its frames of max(M, F+1)+1. */
long long speechPlayer_batch_utteranceSamples(speechPlayer_batch_t batch, long long utterance);
/* The same for every utterance at once: returns the number of utterances, and fills lengths[] when it is <= capacity. */
long long speechPlayer_batch_lengths(speechPlayer_batch_t batch, long long* lengths, long long capacity);
long long speechPlayer_batch_totalSamples(speechPlayer_batch_t batch);
long long speechPlayer_batch_totalFrames(speechPlayer_batch_t batch);
int speechPlayer_batch_sampleRate(speechPlayer_batch_t batch);

/* Launch the synthesis kernel on the batch's stream (asynchronous), and wait for it. */
int speechPlayer_batch_synthesize(speechPlayer_batch_t batch);
int speechPlayer_batch_wait(speechPlayer_batch_t batch);

/* Copy utterance u's PCM to the host (after wait). Returns samples copied (<= capacity). */
long long speechPlayer_batch_read(speechPlayer_batch_t batch, long long utterance, sample* sampleBuf, long long capacity);
/* The same as float samples in [-1, 1] (value / 32767, the scaling of the reference's audio sink,
 * lavPlayer.py:17); the conversion runs on the device. Returns samples copied. */
long long speechPlayer_batch_readFloat(speechPlayer_batch_t batch, long long utterance, float* sampleBuf, long long capacity);
/* Copy every utterance's PCM, concatenated in utterance order; outStart[nUtterances+1] receives
 * the offsets. Returns total samples. */
long long speechPlayer_batch_readAll(speechPlayer_batch_t batch, sample* sampleBuf, long long capacity, long long* outStart);
/* The two large transfers of a batch -- frames in (speechPlayer_batch_setUtterances), PCM out (speechPlayer_batch_readAll) -- run
 * as ONE DMA at the link's rate when the host side is page-locked memory: from speechPlayer_hostAlloc (freed with
 * speechPlayer_hostFree), or memory the caller registered itself (hipHostRegister).  Pageable buffers work as before, through
 * bounce buffers.  The PCM is put into dense utterance order ON THE DEVICE first (the pool pads utterances to 32 samples), so the
 * bytes that cross the link are the bytes of the caller's buffer.  (Additive: the reference has one stream per handle and copies
 * through speechPlayer_synthesize, src/speechPlayer.cpp:41-45.) */
void* speechPlayer_hostAlloc(long long bytes);
void speechPlayer_hostFree(void* p);
/* speechPlayer_batch_readAll without waiting: compaction and copy are queued behind the synthesis and run beside whatever is launched
 * next; sampleBuf must be page-locked (else -1).  Returns the samples that will have arrived when speechPlayer_batch_readWait returns. */
long long speechPlayer_batch_readAllAsync(speechPlayer_batch_t batch, sample* sampleBuf, long long capacity, long long* outStart);
int speechPlayer_batch_readWait(speechPlayer_batch_t batch);
/* Digest of the PCM, computed on the device (for checks of batches whose PCM is too large to copy): perUtterance[u]
 * (may be NULL) = sum over utterance u's samples of mix64(position, value), *whole (may be NULL) = a digest of those in
 * utterance order.  Equal PCM <=> equal digests (up to 2^-64); the kernel is an HBM-bound read of the pool. */
int speechPlayer_batch_digest(speechPlayer_batch_t batch, unsigned long long* perUtterance, unsigned long long* whole);
/* speechPlayer_getLastIndex for utterance u after the run. */
int speechPlayer_batch_getLastIndex(speechPlayer_batch_t batch, long long utterance);

/* Zero-copy access for GPU consumers: device pointer of the PCM pool and the sample offset of
 * utterance u in it (offsets are padded to 64-sample boundaries). */
const sample* speechPlayer_batch_devicePcm(speechPlayer_batch_t batch);
long long speechPlayer_batch_deviceOffset(speechPlayer_batch_t batch, long long utterance);

/* Measurement: run `launches` synthesis launches back to back on the batch's stream and report
 * each launch's duration in milliseconds from HIP events recorded on that stream. */
int speechPlayer_batch_time(speechPlayer_batch_t batch, int launches, float* msPerLaunch);

/* Kernel resource facts for reports: fills vgprs, ldsBytes, wavefronts launched, workgroups per CU. */
int speechPlayer_batch_kernelInfo(speechPlayer_batch_t batch, int* info, int nInfo);
/* info[12..15] (nInfo >= 16): utterances that take their coefficients from tracks, distinct tracks of the batch, their size in
 * MB, 1 if the reported kernel is the tracked (flat-stage) instantiation.
 * info[16..19] (nInfo >= 20): utterances on the direct stages, 1 if the reported kernel is the direct one, the size in MB of the
 * per-frame seeds every launch writes (1376 + 128 bytes per frame of those utterances), 0. */

/* Host-only view of the track planning of speechPlayer_batch_setUtterances (tests, tools; touches no device):
 * the plan for these utterances under a budget of budgetMB.  eligible[u] != 0: utterance u may be tracked (NULL: all; the
 * engine itself tracks the noisy utterances whose parameters are all finite).  Per frame: first entry and mask of the entry
 * kinds that move (bits 0..13: N0, NP, c6..c1, p1..p6; 14..23: pairs of gains) of its fade's track; per utterance: tracked or not (nothing is, once a tenth of the
 * eligible utterances did not fit).  Returns the number of distinct tracks, *nEntries their 16-byte entries; -1 on bad
 * arguments.  A fade's end points follow reference src/frame.cpp:55-72; equal fades share a track. */
long long speechPlayer_planTracks(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
	const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible, long long budgetMB,
	unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked, unsigned long long* nEntries);

/* The same with the per-frame facts GIVEN (facts24: nFrames x 24 bytes as speechPlayer_frameFacts writes them; NULL: computed) and with
 * the check the engine makes of every frame the planner recognised by its 128-bit hash: its 45 shape values compared with those of the
 * first frame that carried the hash (on the device in speechPlayer_batch_setUtterances -- klatt_verify_shared --, here on the host).
 * Returns -2 and the frame in *collisionAt when two frames share a hash and differ (a test forges such facts; the engine then plans
 * the batch again without tracks and leaves a message in speechPlayer_lastError with the call succeeding). */
long long speechPlayer_planTracksFacts(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
	const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible, long long budgetMB, const void* facts24,
	unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked, unsigned long long* nEntries, long long* collisionAt);
/* speechPlayer_planTracks, and per utterance the word of entry kinds the flat stages are told to follow (kinds[nUtterances], may be NULL;
 * the bits of trackMask): every kind some fade of the utterance moves, and every kind whose value the first sample of a later fade
 * re-sets -- the frame after a silence starts from its own values.  0 for an utterance that is not tracked.  Touches no device. */
long long speechPlayer_planTrackKinds(long long nUtterances, const long long* frameStart, const speechPlayer_frame_t* frames,
	const unsigned int* fadeDuration, const unsigned char* isNull, const unsigned char* eligible, long long budgetMB,
	unsigned long long* trackOff, unsigned int* trackMask, unsigned char* tracked, unsigned long long* nEntries, unsigned int* kinds);
/* Host-only view of the fade end points speechPlayer_batch_setUtterances derives for the utterances it sends to the direct stages
 * (tests; touches no device; follows reference src/frame.cpp:55-72): per frame the frames its fade starts from and ends on
 * (0xFFFFFFFF: none -- all values zero) and flags (bit 0: the start's preFormantGain is gated off -- silence --, bit 1: the end's).
 * Returns the number of frames; -1 on bad arguments. */
long long speechPlayer_planDirect(long long nUtterances, const long long* frameStart, const unsigned char* isNull,
                                  unsigned int* from, unsigned int* to, unsigned int* flags);
/* What speechPlayer_batch_setUtterances learns of every frame before it plans a batch (tests, tools): per frame 24 bytes --
 * {u64 h0, u64 h1: a 128-bit hash of the 45 values a track depends on (every parameter but the two pitches), u32 flags, u32 0};
 * flags: 1 a noise gain is set or the parallel bank's coefficients may not be finite, 2 a parameter is NaN or infinite, 4 the nasal
 * pair is coupled in (or could not be skipped safely), 8 a frequency or bandwidth outside the direct stages' range.  onDevice = 0: the
 * host's evaluation (touches no device); 1: the device's (klatt_frame_facts: what frames arriving from page-locked memory get) -- the
 * same function (csrc/klatt_plan.h), the same bytes.  Returns nFrames, -1 on error. */
long long speechPlayer_frameFacts(const speechPlayer_frame_t* frames, long long nFrames, int sampleRate, int onDevice, void* facts24);

/*
 * One batch over the GPUs of a node.  Utterances are independent (the reference's only cross-handle coupling
 * is rand(), src/speechWaveGenerator.cpp:40, replaced by per-utterance noise streams), so the batch is cut into contiguous
 * shards of near-equal total SAMPLE count, one per device; one host thread per device uploads its shard, the devices
 * synthesise side by side, nothing is exchanged between them.  Results are addressed by the batch's own utterance numbers.
 *   devices[nDevices]  HIP device of each shard (NULL: 0 .. nDevices-1; a device may be listed more than once)
 */
typedef void* speechPlayer_node_t;
speechPlayer_node_t speechPlayer_node_create(int sampleRate, int nDevices, const int* devices);
void speechPlayer_node_destroy(speechPlayer_node_t node);
int speechPlayer_node_devices(speechPlayer_node_t node);
int speechPlayer_node_setOption(speechPlayer_node_t node, const char* name, int value);
/* Arguments as speechPlayer_batch_setUtterances; noiseSeed NULL = the utterance's number in the WHOLE batch. */
int speechPlayer_node_setUtterances(speechPlayer_node_t node, long long nUtterances, const long long* frameStart,
	const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, const unsigned int* noiseSeed);
/* The node's batch in compact form (speechPlayer_batch_setRecords, speechPlayer_batch_setIpa / _setIpaVoices): lists, records and the shape
 * table go to every shard, the deal decides which utterances each shard speaks.  sampleRate: the node's (as given to speechPlayer_node_create);
 * voiceOf NULL: voiceName for every text (NULL / "": none). */
int speechPlayer_node_setRecords(speechPlayer_node_t node, long long nShapes, const speechPlayer_frame_t* shapes, long long nLists,
	const long long* listStart, const speechPlayer_frameRecord_t* records, long long nUtterances, const unsigned int* listOf,
	const unsigned int* noiseSeed);
int speechPlayer_node_setIpa(speechPlayer_node_t node, int sampleRate, long long nTexts, const char* const* ipaUtf8, double speed,
	const double* basePitch, double inflection, const char* clauseTypes, const int* voiceOf, const char* voiceName,
	double trailingSilenceMs, const unsigned int* noiseSeed);
int speechPlayer_node_synthesize(speechPlayer_node_t node);   /* asynchronous on every device */
int speechPlayer_node_wait(speechPlayer_node_t node);
long long speechPlayer_node_totalSamples(speechPlayer_node_t node);
long long speechPlayer_node_read(speechPlayer_node_t node, long long utterance, sample* sampleBuf, long long capacity);
int speechPlayer_node_getLastIndex(speechPlayer_node_t node, long long utterance);
/* Option "deal" (besides the batch options, which go to every shard): 0 (default) contiguous shards of near-equal total sample count;
 * 1 the SORTED deal of SURVEY 8(e) -- utterances sorted by length, blocks of 64 (one wavefront) dealt round-robin -- so that every
 * device sees the same length distribution whatever the order of the batch (the shards' frames are then gathered on the host).
 * Shard `shard`: its first utterance (-1 under the sorted deal: its utterances are not a range), utterance count, sample count and
 * device (each pointer may be NULL); speechPlayer_node_shardUtterances lists the shard's utterances in the shard's own order
 * (returns their number; fills when it is <= capacity). */
int speechPlayer_node_shardInfo(speechPlayer_node_t node, int shard, long long* firstUtterance, long long* nUtterances, long long* samples, int* device);
long long speechPlayer_node_shardUtterances(speechPlayer_node_t node, int shard, long long* utterances, long long capacity);
/* The shard's own batch object, for everything else (digest, float output, device pointers); utterance numbers are
 * relative to the shard's first utterance there. */
speechPlayer_batch_t speechPlayer_node_part(speechPlayer_node_t node, int shard);
/* `launches` passes over the whole batch, all devices at once; wall-clock milliseconds per pass. */
int speechPlayer_node_time(speechPlayer_node_t node, int launches, float* msPerLaunch);

/*
 * Many LIVE streams on one GPU: advance nHandles handles created by
 * speechPlayer_initialize by up to sampleCount samples each in ONE kernel launch, one handle per
 * wavefront lane.  Exactly equivalent to calling speechPlayer_synthesize(handles[i], sampleCount,
 * sampleBufs[i]) for every i (queued frames, purge requests, index marks and saved state are per handle);
 * produced[i] receives each call's return value.  Handles must be distinct and share sample rate.
 * The reference's consumer loop is one thread per stream pulling 8192 samples
 * (nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:62-81); this is that loop for N streams.
 * Host cost per call: one control block (44 bytes per handle) and the frames queued since the last call travel, nothing else --
 * a handle's saved state and its queued frames live in a per-device arena (speechPlayer_queueFrame writes a frame once, into a
 * pinned log; a scatter kernel places the log's entries in the handles' rings).  Listing the handles in ascending order of
 * creation saves a sort.
 */
int speechPlayer_synthesizeMany(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, sample** sampleBufs, int* produced);
/* The same with the PCM left in HBM: handle i's samples start at *devicePcm + i * *rowStride.  The pointer is the engine's own pull
 * buffer: it dies at the next live call on that device (the next pull overwrites it) and at "live_trim" (which frees it).
 * speechPlayer_synthesizeManyExport below is the caller-owned form.  For measuring the engine without the PCIe copy of the PCM. */
int speechPlayer_synthesizeManyDevice(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, const sample** devicePcm,
	long long* rowStride, int* produced);
/*
 * speechPlayer_synthesizeMany with handle i's samples written to CALLER-OWNED device memory of the handles' device: row i at element
 * i * rowStride, format 0 int16 / 1 float32 (= sample / 32767, the bits of speechPlayer_batch_exportPcm), elements produced[i] ..
 * rowStride-1 zero; rowStride 0 means sampleCount, and a rowStride below sampleCount is refused.  deviceOut is aligned to the element
 * size (16-byte alignment takes the vector stores).  The pull is unchanged: host-synchronous, produced[] and the index marks are there on
 * return.  The rows are written on `stream` (a hipStream_t of that device; NULL: the null stream) behind an event recorded after the
 * pull, with no host wait; the next live call on the device waits for them on the device before it overwrites the pull buffer, and
 * "live_trim" waits for them before it frees it.  Refused with SPEECHPLAYER_ERR_ARGUMENT before anything is pulled: what
 * speechPlayer_synthesizeMany refuses, an unknown format, a rowStride below sampleCount, and deviceOut that is not device memory of the
 * handles' device, not aligned, or too small.  0, or -1.
 */
int speechPlayer_synthesizeManyExport(speechPlayer_handle_t* handles, int nHandles, unsigned int sampleCount, void* deviceOut,
	int format, long long rowStride, void* stream, int* produced);
/*
 * Queue frames into many live handles in one call.  Exactly: for every i, for k = frameStart[i] .. frameStart[i+1]-1 in order,
 *   speechPlayer_queueFrame(handles[i], isNull && isNull[k] ? NULL : &frames[k], minFrameDuration[k], fadeDuration[k],
 *                           userIndex ? userIndex[k] : -1, purge && purge[i] && k == frameStart[i]).
 * userIndex, isNull and purge may be NULL (frames too, when every frame is NULL); a row whose isNull is set is never read.  The handles
 * may live on different devices.  All or nothing: the call checks everything before it queues anything, and refuses an invalid handle,
 * a handle listed twice, a frameStart that does not run from 0 without decreasing, and a purge[i] set on a handle given no frames --
 * SPEECHPLAYER_ERR_ARGUMENT, no handle's queue changed.  speechPlayer_queueFrame is this call with one handle and one frame.  0, or -1
 * (SPEECHPLAYER_ERR_ARGUMENT / _HIP).
 */
int speechPlayer_queueFramesMany(const speechPlayer_handle_t* handles, int nHandles, const long long* frameStart,
	const speechPlayer_frame_t* frames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, const unsigned char* purge);
/*
 * The same with the 47-double frames in DEVICE memory of the handles' device (a torch tensor); every other array stays on the host.
 *   deviceFrames[frameStart[nHandles]]  8-byte aligned device memory; read before the call returns: then the caller may free or
 *                              overwrite it.  A frame that fits in its handle's ring (256 frames) is placed there by a kernel
 *                              (live_place): 16 bytes of meta, a row number and a target cross the link instead of the 400-byte log entry.
 *                              Frames beyond a ring wait on the host as in speechPlayer_queueFrame: only their rows are gathered on the
 *                              device and downloaded.
 *   readyStream                as in speechPlayer_batch_setUtterancesDevice: a hipStream_t on which the frames are being produced (the
 *                              engine's stream waits for an event recorded there); NULL: the frames are ready.
 * Refused besides, with nothing queued: handles on different devices, and frames that are not device memory of the handles' device
 * (host memory, page-locked or not, included), not 8-byte aligned, or running past the end of their allocation.
 */
int speechPlayer_queueFramesManyDevice(const speechPlayer_handle_t* handles, int nHandles, const long long* frameStart,
	const speechPlayer_frame_t* deviceFrames, const unsigned int* minFrameDuration, const unsigned int* fadeDuration,
	const int* userIndex, const unsigned char* isNull, const unsigned char* purge, void* readyStream);
/* The HIP device a live handle's state lives on (-1: not a handle). */
int speechPlayer_handleDevice(speechPlayer_handle_t handle);
/* Kernel time in milliseconds of the last live call on HIP device `device` (HIP events on its stream). */
float speechPlayer_lastLiveKernelMs(int device);
/* Kernel launches that call took: 1, unless a handle had more frames queued than the 256 its device-side ring holds and the
 * ring's frames ended before sampleCount samples -- such a call proceeds in pieces, with the same result. */
int speechPlayer_lastLiveLaunches(int device);
/* Process-wide options.  "live_layout": the kernel that advances live handles -- 1 (default): the stage-parallel kernel, four
 * wavefronts per 64 handles; 0: the lane kernel, one wavefront per 64 handles.  Same saved state, same PCM.
 * "live_cus": pulls of more than live_cus x 64 handles take the two-workgroups-per-CU instantiation of the stream kernel (0, default:
 * the device's CU count -- 16 384 handles on MI355X; a small value lets a test reach that kernel with a few hundred handles).
 * Memory: every live handle owns a slot of ~100 KB of HBM in a per-device arena (a ring of 256 queued frames with their durations
 * and a 240-double state block); the arena doubles when the slots run out (old and new coexist during the move: ~2.4 GB transient
 * at 16 384 slots), and speechPlayer_initialize fails with SPEECHPLAYER_ERR_HIP when the device cannot hold it.  It does not shrink while
 * a handle lives; "live_trim" = 1 releases a device's arena (and the pull buffers) when the LAST handle on that device is terminated --
 * and at once on devices where none lives; 0 (default) keeps it for the next handles.
 * "live_replicate" (default 1): a pull of fewer than 32 handles fills the empty lanes of their wavefront with replicas of them (a sparse
 * wavefront runs up to 1.7 times slower), and ONE handle pulled alone is advanced in all 64 lanes by a kernel instantiation of its own that
 * computes its fades side by side across the lanes; 0: one lane per handle.  Same PCM, marks and counts either way.
 * "live_mode" (default 0): the arithmetic mode of handles created FROM NOW ON -- 0 MODE_EXACT (the reference's rounding, sample for sample),
 * 1 MODE_FAST (the filters' multiply-adds fused; within north_star's tolerance, held to <= 1 LSB and <= 5 one-LSB differences per million
 * samples against the oracle like the batches' MODE_FAST; one stream 1.27 -> 1.18 ms per 8192-sample pull).  Handles pulled together must share it.
 * "live_alone" (default 1536; 1: only a handle pulled alone): a pull of up to this many handles gives EVERY handle a wavefront of its own
 * (one workgroup per handle, 256 side by side on MI355X, further ones in rounds): handles that share a wavefront pay for one another --
 * unrelated handles 11.2 ms per 8192-sample pull however few they are -- while 2 .. 256 handles alone in their wavefronts take 1.4-1.7 ms
 * and 1024 take 6.2, 1536 9.3 (the two policies meet near 1850 handles).  Handles that speak IN STEP (same frames from the same sample) are the exception: beyond 256 of them sharing
 * wavefronts is faster (2.5 ms) -- set 1 for those.  Needs "live_replicate" 1 and "live_layout" 1.
 * "plan_hash_bits" (tests): how many bits of a frame's 128-bit shape hash the track planner looks at (default 128).
 * Options may be set from any thread; a pull in flight finishes under the values it started with. */
int speechPlayer_setGlobalOption(const char* name, int value);
/* Choose a handle's noise stream (default 0); see DESIGN.md "Noise". */
int speechPlayer_setNoiseSeed(speechPlayer_handle_t playerHandle, unsigned int seed);

/*
 * The frame producer: IPA text -> the frame stream a caller would queue.  Host code, no GPU needed.
 * Native counterpart of the reference's ipa.generateFramesAndTiming (ipa.py:336-353, with :39-334 behind it) and of the
 * NVDA driver's voice presets (nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:86-125); same values for the same input.
 *   clauseType   '.', ',', '?', '!' or 0 (none: the statement contour), as the reference's clauseType argument
 *   voiceName    NULL / "" for none, else one of speechPlayer_voiceName(0 .. speechPlayer_voiceCount()-1); the preset is
 *                applied to every non-silence frame: absolute values first, then multipliers (applyVoiceToFrame)
 */
/* One utterance.  Returns its number of frames n; fills the arrays (each may be NULL) when n <= capacity.  isNull[k] != 0
 * marks silence (the reference yields None); durations are in MILLISECONDS as the reference yields them.  -1: unknown voice;
 * -2: a clauseType the intonation table does not hold (the reference raises KeyError, ipa.py:281). */
long long speechPlayer_ipa_frames(const char* ipaUtf8, double speed, double basePitch, double inflection, int clauseType,
	const char* voiceName, speechPlayer_frame_t* frames, unsigned char* isNull, double* durationMs, double* fadeMs, long long capacity);
/* Many utterances, packed as speechPlayer_batch_setUtterances takes them: durations converted to samples the way the
 * reference wrapper does (speechPlayer.py:53), each utterance followed by silence of trailingSilenceMs (fade 0) as
 * test_speakIpa.py:27 queues it (negative: none).  basePitch[nTexts] may be NULL (100 Hz), clauseTypes[nTexts] may be NULL
 * (none).  Returns the total number of frames; writes frameStart[nTexts+1] when given, and the frame arrays when all four
 * are given and frameCapacity suffices (call once with NULL arrays to size them).  Distinct (text, clause, pitch)
 * combinations are built once per call and instanced.  -1: bad arguments or unknown voice; -2: unknown clause type. */
long long speechPlayer_ipa_pack(int sampleRate, long long nTexts, const char* const* ipaUtf8, double speed, const double* basePitch,
	double inflection, const char* clauseTypes, const char* voiceName, double trailingSilenceMs,
	long long* frameStart, speechPlayer_frame_t* frames, unsigned int* minFrameDuration, unsigned int* fadeDuration,
	unsigned char* isNull, long long frameCapacity);
/* Text in, batch resident in HBM: the producer's compact form (distinct (text, clause, base pitch, voice) combinations built once, as
 * lists of 32-byte records over a table of (voice, phoneme) shapes) handed to speechPlayer_batch_setRecords. */
int speechPlayer_batch_setIpa(speechPlayer_batch_t batch, long long nTexts, const char* const* ipaUtf8, double speed,
	const double* basePitch, double inflection, const char* clauseTypes, const char* voiceName, double trailingSilenceMs,
	const unsigned int* noiseSeed);
/* The same with a voice PER TEXT: voiceOf[i] = index of text i's voice (0 .. speechPlayer_voiceCount()-1; -1 none); NULL: none.
 * BASELINE configs[4] -- 256 voice-parameter variants x 16 384 utterances -- is this call with 256 defined voices. */
int speechPlayer_batch_setIpaVoices(speechPlayer_batch_t batch, long long nTexts, const char* const* ipaUtf8, double speed,
	const double* basePitch, double inflection, const char* clauseTypes, const int* voiceOf, double trailingSilenceMs,
	const unsigned int* noiseSeed);
/* The compact form itself, for callers that keep a batch's description (and for the tests): an object that owns the arrays
 * speechPlayer_batch_setRecords takes.  NULL on bad arguments. */
typedef void* speechPlayer_records_t;
typedef struct {
	long long nShapes; const speechPlayer_frame_t* shapes;
	long long nLists; const long long* listStart;
	long long nRecords; const speechPlayer_frameRecord_t* records;
	long long nUtterances; const unsigned int* listOf;
} speechPlayer_recordsView_t;
speechPlayer_records_t speechPlayer_ipa_records(int sampleRate, long long nTexts, const char* const* ipaUtf8, double speed, const double* basePitch,
	double inflection, const char* clauseTypes, const int* voiceOf, const char* voiceName, double trailingSilenceMs);
int speechPlayer_records_view(speechPlayer_records_t records, speechPlayer_recordsView_t* view);
void speechPlayer_records_free(speechPlayer_records_t records);
/*
 * Phoneme alignment: which phoneme is sounding when.  Beside every record the producer keeps a 16-byte LABEL -- what its lexer knew
 * about the frame -- and a batch set from IPA text carries the labels of its lists to the device, where two exports turn them into
 * framewise labels and a segment table on the caller's stream (klatt_align.h).
 *   phoneme     row of speechPlayer_ipa_phoneme; an inserted pre-stop gap: speechPlayer_ipa_phonemeCount() (SPEECHPLAYER_LABEL "gap" id),
 *               a silence frame (the trailing silence, speechPlayer_batch_setText's pause): count + 1.  Never negative.  A post-stop
 *               aspiration carries the row it is a copy of (/h/) and SPEECHPLAYER_LABEL_PUFF.
 *   flags       SPEECHPLAYER_LABEL_* below: the stress in bits 0-1, then the producer's prosodic bits
 *   unit        index within the utterance of the text symbol the frame belongs to: a gap belongs to the stop after it, an aspiration
 *               to the stop before it, silence is a unit of its own; non-decreasing along a list
 *   textOffset  byte offset in the caller's UTF-8 string at which the symbol begins (after a tie bar that joins two symbols into one
 *               table row: the first of them); -1 for inserted frames and silence.  speechPlayer_batch_setText: always -1 (the IPA
 *               of a clause is eSpeak's, not the caller's string; units count on through the clauses of a text).
 */
typedef struct {
	int phoneme;
	unsigned int flags;
	int unit;
	int textOffset;
} speechPlayer_frameLabel_t;
enum {
	SPEECHPLAYER_LABEL_STRESS_MASK    = 3,     /* 0 none, 1 primary, 2 secondary (set on the syllable's head) */
	SPEECHPLAYER_LABEL_TIED_TO        = 4,     /* a tie bar follows the symbol */
	SPEECHPLAYER_LABEL_TIED_FROM      = 8,     /* a tie bar precedes it */
	SPEECHPLAYER_LABEL_LONG           = 16,    /* a length mark follows it */
	SPEECHPLAYER_LABEL_WORD_START     = 32,
	SPEECHPLAYER_LABEL_SYLLABLE_START = 64,
	SPEECHPLAYER_LABEL_GAP            = 128,   /* the frame is an inserted pre-stop gap; in a unit table: the unit has one */
	SPEECHPLAYER_LABEL_PUFF           = 256    /* ... an inserted post-stop aspiration */
};
/* One utterance's labels, host only (no GPU): the arguments of speechPlayer_ipa_frames that decide the frame list, and the same n
 * frames.  Any array may be NULL; filled when n <= capacity.  Returns n; -1 on an allocation failure. */
long long speechPlayer_ipa_labels(const char* ipaUtf8, int* phoneme, unsigned int* flags, int* unit, int* textOffset, long long capacity);
/* The labels of a records object: *labels is parallel to its view's `records` array (owned by the object).  0, or -1. */
int speechPlayer_records_labels(speechPlayer_records_t records, const speechPlayer_frameLabel_t** labels, long long* nLabels);
/* speechPlayer_batch_setRecords with labels[listStart[nLists]] attached (NULL: none -- the call is then speechPlayer_batch_setRecords).
 * speechPlayer_batch_setIpa, _setIpaVoices and _setText attach theirs; a batch set any other way has none, and any set call without
 * labels drops them.  Refused (the previous batch stays): a list whose units do not count from 0 and rise by at most one from frame to
 * frame, a negative phoneme id. */
int speechPlayer_batch_setRecordsLabelled(speechPlayer_batch_t batch, long long nShapes, const speechPlayer_frame_t* shapes,
	long long nLists, const long long* listStart, const speechPlayer_frameRecord_t* records, const speechPlayer_frameLabel_t* labels,
	long long nUtterances, const unsigned int* listOf, const unsigned int* noiseSeed);
int speechPlayer_batch_hasLabels(speechPlayer_batch_t batch);     /* 1, 0; -1: no batch */
/*
 * speechPlayer_batch_exportAlignment: framewise labels of chosen utterances (any order, repeats; NULL: all) at the steps
 * phase + j * hop, as [row][step][column] of int64 (format 0) or int32 (format 1) in the caller's device memory, on the caller's
 * stream, with the contract of speechPlayer_batch_exportTracks (no synthesis launch, ordered by events, the next set call waits on the
 * device).  rowStride > 0: every row has rowStride steps, `pad` past the utterance's end; 0: the rows back to back.  `capacity`: elements
 * deviceOut holds.  Columns:
 */
#define SPEECHPLAYER_ALIGN_PHONEME     0   /* the label's phoneme id */
#define SPEECHPLAYER_ALIGN_STRESS      1   /* flags & 3 */
#define SPEECHPLAYER_ALIGN_FLAGS       2
#define SPEECHPLAYER_ALIGN_UNIT        3
#define SPEECHPLAYER_ALIGN_TEXT_OFFSET 4
#define SPEECHPLAYER_ALIGN_FRAME       5   /* the request in effect: SPEECHPLAYER_TRACK_FRAME */
#define SPEECHPLAYER_ALIGN_POSITION    6   /* samples since the unit began */
#define SPEECHPLAYER_ALIGN_REMAINING   7   /* samples until the next unit begins (the utterance's end for the last) */
#define SPEECHPLAYER_ALIGN_COLUMNS     8
/* The request in effect on sample t is the last one dequeued on or before t (the utterance's last sample belongs to its last request).
 * Returns the number of elements written, -1 and nothing written when refused (SPEECHPLAYER_ERR_ARGUMENT): no batch, no labels on this
 * batch, a column outside 0 .. 7, nColumns <= 0, hop < 1, phase < 0, an utterance outside the batch, rowStride below the largest step
 * count, capacity below the elements needed, deviceOut not device memory of the batch's device. */
long long speechPlayer_batch_exportAlignment(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances,
	const int* columns, int nColumns, long long hop, long long phase, void* deviceOut, int format, long long rowStride, long long pad,
	long long capacity, void* stream);
/* speechPlayer_batch_exportUnits: the segment table, [row][unit][7] of int64 -- phoneme (that of the unit's frame that is neither gap
 * nor aspiration), flags (ORed over the unit's frames), textOffset, firstSample, samples, firstStep, steps: the steps phase + j * hop
 * that fall inside the unit (a row's `steps` sum to its step count).  byFrame != 0: one entry per frame instead of per unit (gaps and
 * aspirations are entries of their own).  rowStride > 0: rowStride entries per row, `pad` in every column past the row's count; 0: back
 * to back.  Same contract and refusals as above. */
#define SPEECHPLAYER_UNIT_COLUMNS 7
long long speechPlayer_batch_exportUnits(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, long long hop,
	long long phase, int byFrame, void* deviceOut, long long rowStride, long long pad, long long capacity, void* stream);
/* Units (byFrame: frames) per chosen utterance, to size the output (host only).  Returns the number of utterances; -1 when refused. */
long long speechPlayer_batch_unitCounts(speechPlayer_batch_t batch, const long long* utterances, long long nUtterances, int byFrame, long long* counts);
/*
 * Optional text front-end: what the NVDA driver does before the frame producer (reference
 * nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:189-234), with eSpeak NG loaded at run time (dlopen of libespeak-ng.so.1, or of
 * $SPEECHPLAYER_ESPEAK_LIB) -- the library links against nothing of it.  PARITY UNPINNED: eSpeak NG is absent from the reference tree
 * and from this image; only the clause splitting, the replacements and the error path are tested.  Without the library every
 * function that needs it returns -3 (speechPlayer_text_available: 0) and speechPlayer_lastError() says what to install;
 * IPA input (speechPlayer_batch_setIpa) never needs it.
 *   speechPlayer_text_clauses   split text where white space follows one of . ? ! , : ; (:84, :189); per clause its byte range
 *                               [begin, end) in textUtf8, its type ('.', '!', '?', ',' or 0) and the pause after it in ms (:195-205);
 *                               returns the number of clauses (fills up to `capacity` of them; any array may be NULL)
 *   speechPlayer_text_fixups    the four replacements of :214-217 and the strip of :218; returns the bytes needed with the NUL
 *   speechPlayer_text_toIpa     one clause through espeak_TextToPhonemes (UTF-8 in, mode word 0x36100 + 0x82 as :210) + the fix-ups
 *   speechPlayer_batch_setText  one utterance per text: its clauses' frame streams one after the other (clause type per clause),
 *                               then silence of the last clause's pause / speed with a fade of max(10, 10 / speed) ms (:234);
 *                               espeakVoice NULL = "en"; basePitch[nTexts] may be NULL (100 Hz); -1 bad arguments, -3 no eSpeak
 */
int speechPlayer_text_available(void);
long long speechPlayer_text_clauses(const char* textUtf8, long long* begin, long long* end, char* clauseType, double* endPauseMs, long long capacity);
long long speechPlayer_text_fixups(const char* ipaUtf8, char* out, long long capacity);
long long speechPlayer_text_toIpa(const char* textUtf8, const char* espeakVoice, char* out, long long capacity);
int speechPlayer_batch_setText(speechPlayer_batch_t batch, long long nTexts, const char* const* textUtf8, const char* espeakVoice, double speed,
	const double* basePitch, double inflection, const char* voiceName, const unsigned int* noiseSeed);
/* The phoneme table the producer is driven by (the reference's data.py, as numbers): entry `index` of
 * speechPlayer_ipa_phonemeCount() -- its IPA symbol (UTF-8, NUL-terminated, symbolCapacity bytes), its 47 parameter values in
 * speechPlayer_frame_t order, which of them the entry sets (bit k of *fieldMask), and its class bits (1 _isVowel, 2 _isVoiced,
 * 4 _isNasal, 8 _isStop, 16 _isLiquid, 32 _isSemivowel, 64 _isAfricate, 128 _copyAdjacent).  Any output may be NULL.  0, or -1. */
int speechPlayer_ipa_phonemeCount(void);
int speechPlayer_ipa_phoneme(int index, char* symbolUtf8, int symbolCapacity, double* values, unsigned long long* fieldMask, unsigned int* classBits);
/* The voice presets of the NVDA driver (reference __init__.py:86-116), by index and by name. */
int speechPlayer_voiceCount(void);          /* presets, then the voices defined with speechPlayer_voiceDefine */
int speechPlayer_voicePresetCount(void);    /* the driver's presets alone: indices 0 .. this - 1 */
const char* speechPlayer_voiceName(int index);
/* Index of a voice by name (-1: none such), and a voice of the caller's own in the presets' form (reference __init__.py:86-116: per
 * parameter an absolute value, a multiplier, or both -- absolute first): entry e sets parameter param[e] (0..46) to absValue[e] unless
 * that is NaN (or absValue NULL), then multiplies it by multiplier[e] unless that is NaN (or multiplier NULL).  Defining a name again
 * replaces its entries; built-in names cannot be redefined.  Returns the voice's index, -1 on bad arguments. */
int speechPlayer_voiceIndex(const char* voiceName);
int speechPlayer_voiceDefine(const char* voiceName, int nEntries, const int* param, const double* absValue, const double* multiplier);
/* reference __init__.py:118-125.  0, or -1 for an unknown voice. */
int speechPlayer_applyVoiceToFrame(speechPlayer_frame_t* frame, const char* voiceName);

const char* speechPlayer_lastError(void);
/* The reference has no error convention (src/speechPlayer.cpp:25-53 return nothing but counts): its
 * speechPlayer_synthesize returns 0 both when the queue has drained and -- here -- when the GPU call failed.
 * This tells the two apart: 0 after a call that succeeded, one of the codes below after one that failed
 * (per calling thread, describes the most recent speechPlayer_* call that can fail). */
#define SPEECHPLAYER_OK 0
#define SPEECHPLAYER_ERR_ARGUMENT 1   /* invalid handle, NULL pointer, inconsistent arrays, limit exceeded */
#define SPEECHPLAYER_ERR_NO_DEVICE 2  /* no HIP device: the engine has no CPU path */
#define SPEECHPLAYER_ERR_HIP 3        /* a HIP runtime call failed (allocation, copy, launch) */
#define SPEECHPLAYER_ERR_TEXT_FRONTEND 4   /* the optional text front-end: eSpeak NG is not installed, or one of its calls failed */
int speechPlayer_lastErrorCode(void);

#ifdef __cplusplus
}
#endif

#endif
