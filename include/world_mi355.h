/*
 * world_mi355.h -- batched, device-resident extension of WORLD's C API for MI355X.
 *
 * The drop-in boundary of this repo is WORLD's own public C ABI (include/world/,
 * one header per reference header, same names/signatures/struct layouts).  Those
 * entry points take HOST pointers, one utterance per call, exactly like the
 * reference (externs/WORLD_v2/src/world/{dio,stonemask,cheaptrick,d4c,synthesis,harvest}.h).
 *
 * This header is the extension underneath them: a batch of utterances whose
 * waveforms and features stay in HBM, processed by the same kernels.  The
 * per-utterance functions are thin wrappers over a batch of one.  Everything is
 * plain C: opaque handles, device pointers as `double*`, sizes as int/int64_t,
 * int error codes (0 = ok) -- no torch, no C++ types.
 *
 * Layout of a batch (B utterances):
 *   x   : double[sum x_length]          concatenated waveforms, utterance u at x_offset[u]
 *   t,f0: double[sum f0_length]         frames concatenated, utterance u at frame_offset[u]
 *   sp,ap: double[sum f0_length][fft_size/2+1]   row-major, same frame order
 *   y   : double[sum y_length]          synthesised waveforms at y_offset[u]
 * with f0_length[u] = GetSamplesForDIO(fs, x_length[u], frame_period)  (dio.cpp:638-640)
 * and  y_length[u]  = int((f0_length-1)*frame_period/1000*fs)+1        (test/synth.cpp:259)
 * unless given explicitly.
 */
#ifndef WORLD_MI355_H_
#define WORLD_MI355_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libworld_mi355.so is built with -fvisibility=hidden; the declarations below are its exported ABI */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define WM_OK 0
#define WM_ERR_HIP 1              /* a HIP runtime call failed; see WorldMi355LastError() */
#define WM_ERR_BAD_ARG 2
#define WM_ERR_UNSUPPORTED_FFT 3  /* fft_size outside {512,1024,2048,4096}; D4C's own size outside {1024,2048,4096,8192} */
#define WM_ERR_NO_DEVICE 4        /* no HIP device: the product path never falls back to CPU */
#define WM_ERR_UNSUPPORTED 5
#define WM_ERR_IO 6                /* a file could not be written (WorldMi355WriteFiles); see WorldMi355LastError() */

typedef struct WorldMi355Context WorldMi355Context;
typedef struct WorldMi355Batch WorldMi355Batch;

/* All option fields of the reference's four option structs in one POD
 * (dio.h:16-23, cheaptrick.h:16-20, d4c.h:16-18, harvest.h:16-20). */
typedef struct {
  int fs;
  double frame_period;        /* ms */
  double f0_floor;            /* DIO / Harvest */
  double f0_ceil;
  double channels_in_octave;  /* DIO */
  int speed;                  /* DIO decimation ratio 1..12 */
  double allowed_range;       /* DIO */
  double q1;                  /* CheapTrick */
  int fft_size;               /* CheapTrick / D4C / Synthesis; 0 = GetFFTSizeForCheapTrick(fs) */
  double d4c_threshold;       /* D4C */
} WorldMi355Params;

/* Defaults as the reference's analysis CLI sets them (test/analysis.cpp:93-203):
 * floor 71, ceil 800, 2 ch/oct, speed 1, range 0.1, q1 -0.15, threshold 0 (NOT 0.85). */
void WorldMi355DefaultParams(int fs, double frame_period, WorldMi355Params* p);

/* The entry points of WORLD's own API (include/world/*.h) return void: a failure inside them (no HIP device, a HIP
 * error, an unsupported size) prints a message and calls abort(), as the reference aborts on bad_alloc.  A host that
 * would rather lose one utterance than the process installs a handler: it is called INSTEAD of abort() with the name
 * of the step that failed, a WM_ERR_* code and WorldMi355LastError()'s text, and the entry point then returns to its
 * caller with its outputs unspecified.  NULL restores abort().  The functions of this header return codes and never
 * call the handler. */
typedef void (*WorldMi355ErrorHandler)(const char* where, int code, const char* message, void* user);
void WorldMi355SetErrorHandler(WorldMi355ErrorHandler handler, void* user);

/* device < 0: current device.  stream == NULL: the legacy default stream (stream 0).  A context and the batches on it
 * are driven by one thread at a time: its randn table, scratch, side streams and events are shared by all its calls. */
int WorldMi355CreateContext(int device, void* hip_stream, WorldMi355Context** out);
/* Every batch of a context must be destroyed before the context: a batch uses the context's stream and tables. */
void WorldMi355DestroyContext(WorldMi355Context* ctx);
int WorldMi355SetStream(WorldMi355Context* ctx, void* hip_stream);
int WorldMi355Synchronize(WorldMi355Context* ctx);
const char* WorldMi355LastError(void);

/* f0_lengths / y_lengths may be NULL (derived as documented above).  For a
 * synthesis-only batch pass x_lengths = NULL and give f0_lengths (+ y_lengths). */
int WorldMi355CreateBatch(WorldMi355Context* ctx, const WorldMi355Params* params, int n_utt,
                          const int* x_lengths, const int* f0_lengths, const int* y_lengths,
                          WorldMi355Batch** out);
void WorldMi355DestroyBatch(WorldMi355Batch* b);
int64_t WorldMi355BatchTotalSamples(const WorldMi355Batch* b);
int64_t WorldMi355BatchTotalFrames(const WorldMi355Batch* b);
int64_t WorldMi355BatchTotalOutputSamples(const WorldMi355Batch* b);
int WorldMi355BatchFftSize(const WorldMi355Batch* b);
const int64_t* WorldMi355BatchSampleOffsets(const WorldMi355Batch* b);  /* host, n_utt+1 */
const int64_t* WorldMi355BatchFrameOffsets(const WorldMi355Batch* b);   /* host, n_utt+1 */
const int64_t* WorldMi355BatchOutputOffsets(const WorldMi355Batch* b);  /* host, n_utt+1 */

/* Stage entry points; every pointer is a DEVICE pointer.  Asynchronous on the
 * context's stream unless stated.  Same meaning as the reference functions:
 *   Dio        dio.cpp:642-647        StoneMask  stonemask.cpp:211-217
 *   CheapTrick cheaptrick.cpp:200-228 D4C        d4c.cpp:337-397
 *   Synthesis  synthesis.cpp:338-397 (synchronises once internally: the pulse count
 *              decides the size of the overlap-add scratch)
 *   Harvest    harvest.cpp:1223-1255
 * refined_f0 of StoneMask must not be the f0 array (WM_ERR_BAD_ARG): the output is cleared first. */
int WorldMi355Dio(WorldMi355Batch* b, const double* x, double* t, double* f0);
int WorldMi355StoneMask(WorldMi355Batch* b, const double* x, const double* t, const double* f0,
                        double* refined_f0);
int WorldMi355CheapTrick(WorldMi355Batch* b, const double* x, const double* t, const double* f0,
                         double* sp);
int WorldMi355D4C(WorldMi355Batch* b, const double* x, const double* t, const double* f0, double* ap);
int WorldMi355Synthesis(WorldMi355Batch* b, const double* f0, const double* sp, const double* ap,
                        double* y);
int WorldMi355Harvest(WorldMi355Batch* b, const double* x, double* t, double* f0);

/* The sample formats of the callers (test/audioio.cpp), over the batch's concatenated samples, DEVICE pointers:
 *   x[i] = pcm[i] / 32768          wavread of a 16-bit file (:236-249); total samples of the batch
 *   pcm[i] = clamp(int(y[i] * 32767), -32768, 32767), the cast truncating towards zero: wavwrite (:160-167);
 *            total output samples of the batch.  A NaN sample writes 0 (the reference's cast is undefined there). */
int WorldMi355SamplesFromPcm16(WorldMi355Batch* b, const int16_t* pcm, double* x);
int WorldMi355SamplesToPcm16(WorldMi355Batch* b, const double* y, int16_t* pcm);

/* Dio -> StoneMask -> CheapTrick -> D4C, as test/analysis.cpp:243-390 chains them. */
int WorldMi355Analyze(WorldMi355Batch* b, const double* x, double* t, double* f0, double* sp,
                      double* ap);
/* Analyze followed by Synthesis of the features it produced -- the round trip BASELINE.json's metric times
 * (test/analysis.cpp then test/synth.cpp on the same utterances).  Same kernels, same results as the two
 * calls; the f0-only first part of Synthesis (time base, pulse list, the host round trip for the pulse
 * count) runs on a second stream beside CheapTrick and D4C instead of after them. */
int WorldMi355AnalyzeSynthesize(WorldMi355Batch* b, const double* x, double* t, double* f0, double* sp,
                                double* ap, double* y);

/* The f0 front end of the two one-call forms above: a property of the batch.  A new batch has (WM_F0_DIO, 1), the chain
 * of test/analysis.cpp.  With WM_F0_HARVEST the chain is Harvest -> [StoneMask ->] CheapTrick -> D4C (-> Synthesis): the
 * composition of the reference's own functions (the reference ships no caller of Harvest), with the same launches and
 * the same bits as the stage entry points called one by one.  refine 1: StoneMask behind the estimator; 0: the
 * estimator's contour is the f0 of the chain.  The stage entry points are not affected.  May be called between any two
 * calls on the batch; Harvest's workspace is made by the first call that needs it (see WorldMi355HarvestWorkspaceBytes).
 * A NULL batch, an estimator other than the two, refine outside {0, 1}, a batch made without x_lengths (the setter):
 * WM_ERR_BAD_ARG before any device call. */
#define WM_F0_DIO 0
#define WM_F0_HARVEST 1
int WorldMi355BatchSetF0Estimator(WorldMi355Batch* b, int estimator, int refine);
int WorldMi355BatchGetF0Estimator(const WorldMi355Batch* b, int* estimator, int* refine);

/* What Harvest's workspace takes from the device for a batch of n_utt utterances of x_lengths samples, in bytes: the sum of
 * the very sizes its set-up allocates, each as the library's allocator rounds it.  Host only: no context, no HIP call.
 * It grows with the batch's 1 ms frames (Harvest analyses at 1 ms whatever p->frame_period says), not with its frames
 * at the caller's hop.  At the default range (71 - 800 Hz: 152 channels, 105 candidates a frame) it is 33 KB per 1 ms
 * frame at 16 kHz and at 48 kHz alike (32 912 and 33 197 bytes, utterances of 10 s and more; 35 KB at 3 s): 25.6 KB of
 * that are the staging slots of the zero-crossing events (152 channels x 4 kinds x 1024 doubles per tile of 1554
 * decimated samples, whole tiles per utterance), 3.4 KB the four candidate arrays, 1.2 KB the raw candidates; about
 * 4.7 MB per batch do not depend on its length.  So a frame at a 5 ms hop costs 165 KB here, against the 16 KB of its
 * fp64 sp + ap rows at fft_size 1024: a batch sized for those (1.5 M frames) would ask for 233 GiB.  Only fs, f0_floor
 * and f0_ceil of p are read.  A NULL argument, n_utt < 1, a length < 1, a range that is none: WM_ERR_BAD_ARG; an f0
 * range Harvest's kernels do not cover (more than 192 candidates a frame): WM_ERR_UNSUPPORTED. */
int WorldMi355HarvestWorkspaceBytes(const WorldMi355Params* p, int n_utt, const int* x_lengths, int64_t* bytes);

/* Per-utterance status of a batch: status[u] (DEVICE pointer, n_utt ints) receives a bit mask.  Utterances of a
 * batch never exchange data, so one with a flag set does not affect the results of the others (SURVEY.md section 5;
 * the reference has no error reporting: every entry point returns void).  x, f0, sp, ap are the arrays of the
 * analysis calls; any of them may be NULL and is then not scanned.  Asynchronous on the context's stream. */
#define WM_UTT_INPUT_NONFINITE 1   /* NaN / Inf among the samples of x */
#define WM_UTT_TOO_SHORT 2         /* f0_length <= Dio's voice_range_minimum: f0 is all zero (dio.cpp:263-266).  Dio's rule:
                                    * never set for a batch whose estimator is WM_F0_HARVEST, which has no such minimum */
#define WM_UTT_OUTPUT_NONFINITE 4  /* NaN / Inf among the utterance's f0 / sp / ap */
#define WM_UTT_D4C_DEFAULT_ROWS 8  /* never set since round 5 (kept for ABI compatibility): it marked frames with f0 >= fs / 16
                                    * at fs above 48.1 kHz, which kept D4C's default row; they are analysed now */
int WorldMi355UtteranceStatus(WorldMi355Batch* b, const double* x, const double* f0, const double* sp,
                              const double* ap, int* status);

/* ---- Feature codec (externs/WORLD_v2/src/codec.cpp), SURVEY.md section 8(f) ---------------------------
 * All arrays are device pointers over the batch's frames (row-major, frame order of the batch).
 *   coded sp : double[total_frames][number_of_dimensions]
 *   coded ap : double[total_frames][WorldMi355GetNumberOfAperiodicities(fs)]
 * fs and fft_size are the batch's. */
int WorldMi355GetNumberOfAperiodicities(int fs);                                  /* codec.cpp:212-215 */
int WorldMi355CodeSpectralEnvelope(WorldMi355Batch* b, const double* sp, int number_of_dimensions,
                                   double* coded);                                /* codec.cpp:268-295 */
int WorldMi355DecodeSpectralEnvelope(WorldMi355Batch* b, const double* coded, int number_of_dimensions,
                                     double* sp);                                 /* codec.cpp:297-324 */
int WorldMi355CodeAperiodicity(WorldMi355Batch* b, const double* ap, double* coded);    /* codec.cpp:217-235 */
int WorldMi355DecodeAperiodicity(WorldMi355Batch* b, const double* coded, double* ap);  /* codec.cpp:237-266 */
/* The coded float32 feature set of the recipe's call `analysis wav lf0 mgc bap 5 2048 50 25`
 * (data/Makefile.in:214, test/analysis.cpp:292-366): lf0[total_frames], mgc[total_frames][spec_dim],
 * bap[total_frames][ap_dim] from resident f0 / sp / ap. */
int WorldMi355RecipeFeatures(WorldMi355Batch* b, const double* f0, const double* sp, const double* ap,
                             int spec_dim, int ap_dim, float* lf0, float* mgc, float* bap);
/* The way back, as the synth CLI does it before Synthesis (test/synth.cpp:151-256):
 *   f0 = exp(lf0), 0 stays 0;  sp = DecodeSpectralEnvelope(mgc with c0 - 12.0) / 1e4;
 *   ap[.][j] = exp(mgc2sp(bap with c0 + 9.210340, order, alpha 0.55, gamma 0)[j]) / 1e4 for j < order,
 *   order = ap_dim (minus one when odd), mgc2sp being the CLI's SPTK port (test/sptkfunctions.cpp:186-274,
 *   :596-631).  The reference leaves bins >= order of every ap row uninitialised (synth.cpp:240-245); they
 *   are written as 0.0 here.  An even ap_dim makes mgc2sp read one coefficient past the row; it is taken as 0.
 *   ap_dim <= 64. */
int WorldMi355RecipeDecode(WorldMi355Batch* b, const float* lf0, const float* mgc, const float* bap, int spec_dim,
                           int ap_dim, double* f0, double* sp, double* ap);

/* ---- Mel-cepstral analysis of spectra: the CLIs' SPTK port, mcep (test/sptkfunctions.cpp:11-184) with flng = fft_size
 * and its solver theq (test/theq.cpp:286-357) -- at gamma 0 what `mgcep -a alpha -m order -l fft_size -q itype` computes
 * from sp / ap (data/Makefile.in:190-206), and what mgc2sp (sptkfunctions.cpp:186-219) inverts.  Fields as mcep's
 * arguments (:11-13): alpha a, order m, itr1 / itr2 the least / most Newton steps (:142-158), dd the end condition
 * (:153), etype 0 nothing or 1 `e` added to the periodogram (:31-33; 2, the dB floor of :104-117, is WM_ERR_UNSUPPORTED),
 * f theq's singularity threshold (theq.cpp:90-104, negative: 1e-6), itype 3 amplitude or 4 periodogram rows (:85-94;
 * 0 / 1 / 2 are WM_ERR_UNSUPPORTED here).  itype 0, windowed frames, and etype 2 are what WorldMi355MelCepstrumOfFrames and
 * WorldMi355MelCepstrumOfWaveform below take, with this same struct. */
typedef struct {
  double alpha;
  int order;
  int itr1, itr2;
  double dd;
  int etype;
  double e;
  double f;
  int itype;
} WorldMi355McepOption;
/* SPTK's defaults: alpha 0.35, order 25, itr1 2, itr2 30, dd 1e-3, etype 0, e 0, f 1e-6, itype 3. */
void WorldMi355DefaultMcepOption(WorldMi355McepOption* opt);
/* spectrum: DEVICE double[total_frames][fft_size/2+1]; mc: DEVICE double[total_frames][order+1];
 * status: DEVICE int[total_frames] or NULL: 0 converged, -1 ran itr2 steps without meeting dd (mcep's own return,
 * :179-182), 1 the solver met a singular pivot (the reference exits the process there, :170-173), 2 a periodogram value
 * <= 0 or non-finite (the reference exits there too, :119-124); rows of status 1 hold the last iterate, rows of
 * status 2 zeros.  Frames never exchange data.  1 <= order <= 63, 0 <= itr1, 0 <= itr2 <= 1000, |alpha| < 1, else
 * WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's stream. */
int WorldMi355MelCepstrum(WorldMi355Batch* b, const double* spectrum, const WorldMi355McepOption* opt, double* mc,
                          int* status);

/* ---- Mel-cepstra from windowed frames and from waveforms: the recipe line that starts at a waveform
 * (data/Makefile.in:134-137),
 *   x2x +sf raw | frame -l L -p P | window -l L -L fft_size -w type -n norm | mgcep -a alpha -m order -l fft_size -e eps
 * at gamma 0, mgcep being mcep (test/sptkfunctions.cpp:11-184) with itype 0, "windowed data sequence" (:66-72): fftr,
 * x[k] = re^2 + im^2 + eps (:68-71), for etype 2 the floor at max 10^(e / 10) (:104-117), then as WorldMi355MelCepstrum.
 * SPTK's frame and window are not in the reference tree; they are taken by this definition:
 *   frame    an utterance of T >= 1 samples x[0 .. T), length L, shift P, 1 <= P <= L <= fft_size, has
 *            J = ceil((T + L / 2) / P) frames (L / 2 rounded down); frame j holds z[i] = x[j P - L / 2 + i], i < L, zero
 *            outside [0, T): frame 0 is centred on sample 0, and frames go on while they hold a sample.  T = 0: J = 0.
 *   window   a = 2 pi / (L - 1); type 0 Blackman 0.42 - 0.5 cos(a i) + 0.08 cos(2 a i), 1 Hamming 0.54 - 0.46 cos(a i),
 *            2 Hanning 0.5 - 0.5 cos(a i), 5 rectangular (3 Bartlett and 4 trapezoid: WM_ERR_UNSUPPORTED); normalize 0 as
 *            it is, 1 scaled to sum w^2 = 1, 2 to sum w = 1; computed in double.  The windowed frame is w[i] z[i], one
 *            multiply, and fft_size - L zeros; with pipe_float32 every product is rounded to float32 once, which is what
 *            SPTK's pipe between `window` and `mgcep` carries.
 * Both host only, no device needed: n_frames of n_samples, or WM_ERR_BAD_ARG outside 1 <= frame_shift <= frame_length or
 * for n_samples < 0; the table w[length], or WM_ERR_BAD_ARG for a type outside 0 .. 5, normalize outside 0 .. 2,
 * length < 2 or a table to be normalised whose sum is not positive. */
int WorldMi355SptkFrames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames);
int WorldMi355SptkWindow(int type, int normalize, int length, double* w);
/* frames: DEVICE double[total_frames][fft_size], windowed and zero-padded; mc, status and their codes as
 * WorldMi355MelCepstrum's (rows of status 2 -- a periodogram value <= 0 or non-finite after eps and the floor -- are zeros).
 * opt->itype must be 0; etype 0, 1 (e >= 0) or 2 (e < 0, :26-29); order, step and alpha limits as WorldMi355MelCepstrum's;
 * anything else is WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's stream. */
int WorldMi355MelCepstrumOfFrames(WorldMi355Batch* b, const double* frames, const WorldMi355McepOption* opt, double* mc,
                                  int* status);
/* The same from the samples: x DEVICE, the batch's packed samples as WorldMi355Dio takes them
 * (WorldMi355BatchSampleOffsets); window HOST double[frame_length] (WorldMi355SptkWindow's, or the caller's own), uploaded
 * by the library; mc DEVICE double[total_frames][order+1].  The batch's f0_lengths must be WorldMi355SptkFrames of its
 * x_lengths, and frame_length <= fft_size, 1 <= frame_shift <= frame_length, else WM_ERR_BAD_ARG before any device call.
 * The frames are gathered, windowed and transformed on the way in: neither they nor their periodograms exist in device
 * memory.  The bits are those of WorldMi355MelCepstrumOfFrames on the frames of the definition above. */
int WorldMi355MelCepstrumOfWaveform(WorldMi355Batch* b, const double* x, const double* window, int frame_length,
                                    int frame_shift, int pipe_float32, const WorldMi355McepOption* opt, double* mc,
                                    int* status);

/* ---- Spectra from mel-generalized cepstra: the CLIs' SPTK port, mgc2sp(mgc, m, a, g, x, y, flng = fft_size)
 * (test/sptkfunctions.cpp:186-219) = mgc2mgc towards alpha 0, gamma 0 and fft_size/2 coefficients (:221-254: freqt
 * :596-631, gnorm :313-328, gc2gc :347-385, ignorm :330-345) and c2sp (:256-274, fftr :387-461) -- what `mgc2sp -a alpha
 * -g gamma -m order -l fft_size` computes, the inverse of WorldMi355MelCepstrum at gamma 0 and the decoder of `mgcep`
 * features at the GAMMA of data/Makefile.in:138-146, 186-192.  Fields as mgc2sp's arguments (:186-187): alpha a, gamma g,
 * order m; out_format 0 ln |H| (the reference's x), 3 |H| = exp(x), 4 |H|^2 = exp(2 x) -- numbered as
 * WorldMi355McepOption.itype, so 3 / 4 here is what itype 3 / 4 takes there.  SPTK's gain-normalized input (-n, -u) and
 * 20 log10 output are not offered. */
typedef struct {
  double alpha;
  double gamma;
  int order;
  int out_format;
} WorldMi355Mgc2spOption;
/* SPTK's defaults: alpha 0.35, gamma 0, order 25; out_format 0. */
void WorldMi355DefaultMgc2spOption(WorldMi355Mgc2spOption* opt);
/* mc: DEVICE double[total_frames][order+1]; spectrum: DEVICE double[total_frames][fft_size/2+1]; phase: the same shape
 * or NULL: the imaginary part y (:216, fftr's sign: that of sum c[n] exp(-2 pi i k n / fft_size)), whatever out_format;
 * status: DEVICE int[total_frames] or NULL: 0 fine, 1 a non-finite coefficient or 1 + gamma c0 <= 0 (c0 after the
 * frequency transformation; the reference's pow returns NaN there, :313-321): such rows are zeros, phase included.
 * Frames never exchange data.  1 <= order <= 63, order <= fft_size/2, |alpha| < 1, -1 <= gamma <= 0, else
 * WM_ERR_BAD_ARG; any other out_format WM_ERR_UNSUPPORTED; both before any device call.  Asynchronous on the context's
 * stream. */
int WorldMi355MelCepstrumToSpectrum(WorldMi355Batch* b, const double* mc, const WorldMi355Mgc2spOption* opt,
                                    double* spectrum, double* phase, int* status);

/* ---- Conversion between mel-generalized cepstra: SPTK's `mgc2mgc`, the step gen_wave (scripts/Training.pl:2861-2868) and
 * postfiltering_lsp (:2702-2705, :2739-2742) take with GAMMA != 0.  Rows c1[0 .. m1] at (alpha a1, gamma g1) become
 * c2[0 .. m2] at (a2, g2).  The core is the CLIs' SPTK port, mgc2mgc(c1, m1, a1, g1, c2, m2, a2, g2)
 * (test/sptkfunctions.cpp:221-254), in its own branches, with a = (a2 - a1) / (1 - a1 a2) in that expression (:238):
 *   a == 0   gnorm(m1, g1) (:313-328), gc2gc(m1, g1 -> m2, g2) (:347-385), ignorm(m2, g2) (:330-345);
 *   a != 0   freqt(m1 -> m2, a) (:596-631), gnorm over M2 coefficients with g1, gc2gc(m2, g1 -> m2, g2), ignorm(m2, g2).
 * The four flags are those of SPTK's command line, which is not in the reference tree.  FLAG SEMANTICS UNPINNED AGAINST
 * SPTK'S COMMAND: the yardstick is this definition, which tests/mgc2mgc_reference.py states in float64.
 *   in_normalized  (-n)  before the core, c <- ignorm(c, m1, g1): c[k] <- K c[k], c[0] <- (K - 1) / g1 with
 *                        K = pow(c[0], g1) (c[0] <- log c[0] at g1 == 0).  Takes precedence over in_multiplied's c[0] rule.
 *   in_multiplied  (-u)  before the core and after -n's step, c[0] <- (c[0] - 1) / g1 (not with -n), then c[k] <- c[k] / g1
 *                        for k >= 1.  WM_ERR_BAD_ARG at g1 == 0.
 *   out_normalized (-N)  after the core, c <- gnorm(c, m2, g2): c[k] <- c[k] / (1 + g2 c[0]),
 *                        c[0] <- pow(1 + g2 c[0], 1 / g2) (c[0] <- exp c[0] at g2 == 0).  Takes precedence over
 *                        out_multiplied's c[0] rule.
 *   out_multiplied (-U)  after the core and after -N's step, c[0] <- c[0] g2 + 1 (not with -N), then c[k] <- c[k] g2 for
 *                        k >= 1.  WM_ERR_BAD_ARG at g2 == 0.
 * The flag steps, gnorm's division and ignorm's product are these expressions without contraction; pow, exp and log are
 * the device library's.  freqt is the reference's expression in its order: at g1 == g2 == 0 without flags c2[1 .. m2] are
 * its bits.  Towards out_order <= 64 gc2gc's sums run in the reference's order with its roundings; towards more
 * coefficients they run in another order and differ from the reference's by its rounding error. */
typedef struct {
  int in_order;             /* m1 */
  double in_alpha;          /* a1 */
  double in_gamma;          /* g1 */
  int in_normalized;        /* -n */
  int in_multiplied;        /* -u */
  int out_order;            /* m2 */
  double out_alpha;         /* a2 */
  double out_gamma;         /* g2 */
  int out_normalized;       /* -N */
  int out_multiplied;       /* -U */
} WorldMi355MgcConvertOption;
/* SPTK's defaults: orders 25, alphas 0, gammas 0, no flag. */
void WorldMi355DefaultMgcConvertOption(WorldMi355MgcConvertOption* opt);
/* in: DEVICE double[total_frames][in_order+1]; out: DEVICE double[total_frames][out_order+1], no element shared with
 * `in`; status: DEVICE int[total_frames] or NULL: 0 fine; 1 a non-finite input coefficient or a gain that is not positive
 * (c[0] itself under in_normalized, else 1 + g1 c0 of the plain row for g1 != 0, and 1 + g1 c2[0] after freqt in the
 * a != 0 branch, where the reference's pow returns NaN); 2 a non-finite result.  Flagged rows are zeros.  Rows never
 * exchange data.  1 <= in_order, out_order <= 4095 with min(in_order, out_order) <= 63, |alpha| < 1 and
 * -1 <= gamma <= 1 on both sides, else WM_ERR_BAD_ARG, as for a NULL `in` or `out` or ranges that share an element; all
 * before any device call.  Timed as "mgc2mgc_kernel".  Asynchronous on the context's stream.
 * Not offered: lpc2lsp (LSP from LPC; the way back is WorldMi355LspToLpc below), mglsadf and mgcep at gamma != 0,
 * WorldMi355MelCepstrumToSpectrum of flagged input, host pointers, min(in_order, out_order) > 63.  The energy sum of
 * postfiltering_lsp is part of WorldMi355LspPostfilter below. */
int WorldMi355MelGeneralizedCepstrumConvert(WorldMi355Batch* b, const double* in, const WorldMi355MgcConvertOption* opt,
                                            double* out, int* status);

/* ---- MGC-LSP rows to MGC rows, and the LSP postfilter.  With GAMMA != 0 the recipe's `mgc` stream holds MGC-LSP rows
 * [gain, lsp_1 .. lsp_m] (data/Makefile.in:138-146, 186-192); gen_wave and postfiltering_lsp (scripts/Training.pl:2690-2752,
 * :2846-2868) take them back by `lspcheck -c -r 0.1 -g -G 1e-10 | lsp2lpc | mgc2mgc -n -u`.  SPTK's lspcheck and lsp2lpc
 * are not in the reference tree.  PARITY WITH SPTK'S COMMANDS IS UNPINNED: the yardstick is the definition below, which
 * tests/lsp_reference.py states in float64.  Everything is in double; the float32 of the commands' pipes and files
 * appears only at the recipe's file ends.  One row is x[0 .. m]: x[0] the gain, w[i] = x[i], i = 1 .. m, radians meant to
 * lie in (0, pi); r = min_distance, G = min_gain, d = r pi / (m + 1) in that expression, pi the double nearest to it.
 *
 * 1. Check (lspcheck -c -r r -g -G G [-L]), the steps in this order, plain expressions without contraction:
 *      range     w <- |w|, then w <- 2 pi - w where w > pi;
 *      order     sorted ascending (the outcome of the command's repeated adjacent swaps);
 *      distance  ONE pass, i = 1 .. m-1 ascending, each step on the values the steps before it left: t = w[i+1] - w[i];
 *                if t < d: s = 0.5 (d - t), w[i] -= s, w[i+1] += s;
 *      gain      K = exp(x[0]) under log_gain (the device library's exp), else x[0].  K < G: K <- G, and the checked row's
 *                gain is log(G) (the host library's log) under log_gain, else G.  Otherwise the gain keeps its bits.
 *    status bits: 1 a range, order or distance step changed a value; 2 the gain was raised; 4 a non-finite input value:
 *    the row and everything derived from it are zeros; 8 a non-finite result: zeros; 16 the checked LSPs are not strictly
 *    increasing inside (0, pi) -- the single pass does not guarantee it; the row is converted all the same.
 * 2. lsp2lpc: A(z) = (P(z) + Q(z)) / 2 with f_i(z) = 1 - 2 cos(w[i]) z^-1 + z^-2, P the product of the f_i of odd i
 *    (1, 3, ...), Q of even i; for even m P takes the further factor (1 + z^-1) and Q (1 - z^-1), for odd m Q takes
 *    (1 - z^-2).  The row is [K, a_1 .. a_m] (a_0 = 1 dropped), K linear whatever log_gain is.  cos is the device
 *    library's.  Order of the products: both start from 1; the quadratic factors of P and of Q are taken in turn, each
 *    polynomial's own in the bit-reversed order of their positions (position j = 0, 1, ... among its factors in ascending
 *    i, sorted by the reversal of j's binary digits over ceil(log2 n) bits: at m = 7, i = 1, 2, 5, 6, 3, 4, 7), each as
 *    c[k] <- (c[k] + p_i c[k-1]) + c[k-2] with p_i = -2 cos(w[i]); then the further factor as c[k] +- c[k-1] (c[k] - c[k-2]);
 *    then a_k = 0.5 (P[k] + Q[k]); no contraction anywhere.  (In ascending i the partial products grow to 1e8 at m = 63
 *    and P + Q keeps no digit; in this order they stay small.)
 * 3. LSP -> MGC (gen_wave, :2861-2868): steps 1 and 2, then WorldMi355MelGeneralizedCepstrumConvert's core on the LPC row
 *    with in_normalized = in_multiplied = 1 at (alpha, gamma) towards (out_order, out_alpha, out_gamma), plain output;
 *    its rules and refusals are unchanged.  gamma < 0 is required.
 * 4. LSP postfilter (postfiltering_lsp, :2690-2752), factor beta = $pf_lsp, length L = $fl (IMPLEN).  From the RAW row,
 *    as the script reads the file itself (:2709): for i = 2 .. m-1, d1 = beta (w[i+1] - w[i]), d2 = beta (w[i] - w[i-1]),
 *      p[i] = w[i-1] + d2 + (d2 d2 ((w[i+1] - w[i-1]) - (d1 + d2))) / ((d2 d2) + (d1 d1)),
 *    p[1] = w[1], p[m] = w[m], all from the unfiltered neighbours in exactly this expression; where d1 == 0 and d2 == 0
 *    (Perl would die) p[i] = w[i].  The script reads the values through `x2x +fa`'s text: that rounding is NOT modelled.
 *    Energies (:2702-2705, :2739-2742): ene = 1/2 ln sum_{k < L} c2[k]^2, c2 being step 3 towards (L - 1, alpha 0, gamma 1)
 *    of the CHECKED row -- the command's output as it is: c2[0] is the gamma = 1 coefficient, not the response's first
 *    sample.  ene1 is of the raw row, ene2 of [gain, p].  The output row is [gain', p], its LSPs NOT checked (the script
 *    merges the .lsp file as written, :2747).  compensation 0 (default) is the script as written: :2745 divides ene2 by
 *    itself, so gain' = gain bit for bit, and no energy is computed unless ene1 / ene2 are asked for.  compensation 1 is
 *    what the two energy files evidently exist for: gain' = gain + (ene1 - ene2) under log_gain, else
 *    gain exp(ene1 - ene2).  beta == 1 or m <= 2 is the identity: rows copied bit for bit, status 0, energies (where
 *    asked for) 0, nothing computed; gen_wave skips the step at 1.0 (:2853).
 *    status: 4 a non-finite input value; 8 a non-finite p, energy or gain', or a row the conversion refuses (its status
 *    1 or 2); such rows and their energies are zeros.  Where energies are computed, bits 1, 2 and 16 of the two checks
 *    are or-ed in; they change nothing in the output row. */
typedef struct {
  int order;                /* m: 1 .. 63 */
  double alpha;             /* of the MGC-LSP stream, |alpha| < 1 */
  double gamma;             /* of the MGC-LSP stream, -1 <= gamma < 0 */
  int log_gain;             /* -L / $lg: x[0] is ln K */
  double min_distance;      /* -r: 0 .. 1 */
  double min_gain;          /* -G: finite, > 0 */
} WorldMi355LspOption;
typedef struct {
  int order;
  double alpha;
  double gamma;
  int log_gain;
  double min_distance;
  double min_gain;
  double beta;              /* $pf_lsp */
  int length;               /* $fl: a power of two, 64 .. 4096 */
  int compensation;         /* 0 the script as written, 1 gain' carries ene1 - ene2 */
} WorldMi355LspPostfilterOption;
/* order 25, alpha 0.35, gamma -1, log_gain 0, min_distance 0.1, min_gain 1e-10; beta 0.7, length 4096, compensation 0. */
void WorldMi355DefaultLspOption(WorldMi355LspOption* opt);
void WorldMi355DefaultLspPostfilterOption(WorldMi355LspPostfilterOption* opt);
/* All three: lsp DEVICE double[total_frames][order+1]; asynchronous on the context's stream; WM_OK on zero frames; rows
 * never exchange data.  WM_ERR_BAD_ARG before any device call for order outside 1 .. 63, not |alpha| < 1, gamma outside
 * [-1, 0), min_distance outside [0, 1], a min_gain that is not finite and positive, a non-finite beta, a length that is no
 * power of two in 64 .. 4096, a NULL required pointer, and ranges that share an element (the postfilter's out may be
 * exactly lsp).  Timed as "lsp_kernel" and "mgc2mgc_kernel".
 * LspToLpc: steps 1 and 2.  lpc DEVICE double[total_frames][order+1]; checked (the checked rows, gain as step 1 leaves it)
 * the same shape or NULL; status DEVICE int[total_frames] or NULL. */
int WorldMi355LspToLpc(WorldMi355Batch* b, const double* lsp, const WorldMi355LspOption* opt, double* lpc,
                       double* checked, int* status);
/* Step 3.  out DEVICE double[total_frames][out_order+1]; status DEVICE int[total_frames], required: step 1's bits, and 8
 * where the conversion flags the row (zeros).  out_order, out_alpha, out_gamma as WorldMi355MgcConvertOption's. */
int WorldMi355LspToMelGeneralizedCepstrum(WorldMi355Batch* b, const double* lsp, const WorldMi355LspOption* opt,
                                          int out_order, double out_alpha, double out_gamma, double* out, int* status);
/* Step 4.  out DEVICE double[total_frames][order+1], or lsp itself; ene1, ene2 DEVICE double[total_frames] or NULL;
 * status DEVICE int[total_frames], required.  The energies are summed inside the conversion kernel as each c2[k] becomes
 * final: no row of `length` coefficients exists in device memory, the call's workspace is two LPC rows and two doubles
 * per frame, and an energy's bits do not depend on how rows are batched. */
int WorldMi355LspPostfilter(WorldMi355Batch* b, const double* lsp, const WorldMi355LspPostfilterOption* opt, double* out,
                            double* ene1, double* ene2, int* status);

/* ---- Waveforms from mel-cepstra: the first branch of gen_wave (scripts/Training.pl:2873-2899), the synthesis half of the
 * recipe's default configuration (USEWORLD = 0, GAMMA = 0),
 *   sopr -m 0 pit | excite -n -p P | dfs -b highpass > unv
 *   excite -n -p P pit | dfs -b lowpass | vopr -a unv | mglsadf -P pd -m order -p P -a alpha -c 0 mgc | x2x +fs -o
 * SPTK is not in the reference tree.  PARITY WITH SPTK IS UNPINNED: the yardstick is the definition below, which
 * tests/mlsa_reference.py states in float64.  Everything is in double unless a float32 pipe is named; T is the number of
 * frames of an utterance, P = frame_shift; an utterance of T >= 2 frames gives (T - 1) P samples.
 *   noise      nrandom at excite's seed: next = 1 (unsigned); rnd(): next = next * 1103515245 + 12345,
 *              r = (next / 65536) % 32768, value r / 32767.0.  Pairs: repeat r1 = 2 rnd() - 1, r2 = 2 rnd() - 1,
 *              s = r1 r1 + r2 r2 while s > 1 or s == 0; s = sqrt(-2 log(s) / s); the pair is r1 s, r2 s.  The sequence
 *              g[0], g[1], ... is the same for every utterance and for both excite processes of the line.
 *   excite     pitch[T]: the period in samples, exactly 0 = unvoiced.  p1 = pitch[0], cnt = p1.  For f = 1 .. T-1, p2 =
 *              pitch[f]: if p1 != 0 and p2 != 0, inc = (p2 - p1) / P, else inc = 0, cnt = p2, p1 = 0.  Then P times: p1 == 0
 *              emits the next unused g; otherwise cnt += 1, and cnt >= p1 emits sqrt(p1) with cnt -= p1, anything else 0;
 *              then p1 += inc.  After the frame p1 = p2.
 *   dfs        y[n] = sum_k b[k] x[n - k], x zero before sample 0, taps taken in the order k = 0, 1, ...
 *   e          e[n] = dfs(lowpass, excite(pitch))[n] + dfs(highpass, g)[n].  Both tap sets are the CALLER's (the recipe's
 *              makefilter.pl prints the ones it uses); the library holds no filter table.
 *   mglsadf    per frame b = mc2b(mc): b[m] = mc[m], b[i] = mc[i] - alpha b[i+1].  Between frames f and f + 1,
 *              inc[k] = (b_next[k] - b[k]) / P and b[k] += inc[k] after every sample, as a running sum; after P samples
 *              b = b_next exactly.  Per sample x = e[n] exp(b[0]), x = mlsadf1(x), y[n] = mlsadf2(x), with
 *              aa = 1 - alpha^2, the Pade row pp[0 .. pd] and all state zero at the start:
 *                mlsadf1  out = 0; for i = pd .. 1: d1[i] = aa pt1[i-1] + alpha d1[i], pt1[i] = d1[i] b[1],
 *                         v = pt1[i] pp[i], x += (i odd) ? v : -v, out += v; then pt1[0] = x, out += x
 *                mlsadf2  the same with pt2[i] = mlsafir(pt2[i-1], D[i-1]) in place of the first two assignments
 *                mlsafir  d[0] = x, d[1] = aa d[0] + alpha d[1]; for k = 2 .. m: d[k] += alpha (d[k+1] - d[k-1]),
 *                         y += d[k] b[k]; for k = m+1 .. 2: d[k] = d[k-1]
 *   Pade rows  pp[0] = 1.  Order 4: 0.4999273, 0.1067005, 0.01170221, 0.0005656279 and order 5: 0.4999391, 0.1107098,
 *              0.01369984, 0.0009564853, 0.00003041721, SPTK's modified tables AS RECALLED.  Orders 1, 2, 3, 6 and 7 are
 *              the plain Pade approximant of exp, pp[k] = L! (2L-k)! / ((2L)! k! (L-k)!): SPTK's own tables for 6 and 7
 *              were not at hand.  Whoever has them passes them in pade[] with use_pade = 1 and gets SPTK's filter.
 *   float32    with pipe_float32 a value is rounded to float32 once at each pipe of the line: excite's output (both
 *              times), each dfs output, the vopr sum and mglsadf's output.
 * Not offered: gamma != 0, an interpolation period other than 1, -k, -t, -v, excite without -n. */
typedef struct {
  double alpha;           /* 0.35 */
  int order;              /* m; 25 */
  int pade_order;         /* pd, 1 .. 7; 4 */
  int frame_shift;        /* P, samples per frame; 100 */
  int pipe_float32;       /* 0 */
  int use_pade;           /* 0: the row of pade_order as above; 1: pade[0 .. pade_order] */
  double pade[8];
} WorldMi355MlsaOption;
void WorldMi355DefaultMlsaOption(WorldMi355MlsaOption* opt);
/* Host only, no device needed.  MlsaSamples: (n_frames - 1) * frame_shift, WM_ERR_BAD_ARG for n_frames < 2, frame_shift < 1
 * or a product beyond int.  MlsaPade: row[0 .. order] of the table above, WM_ERR_BAD_ARG outside 1 .. 7.  MlsaNoise: the
 * first n values of g, WM_ERR_BAD_ARG for n < 0. */
int WorldMi355MlsaSamples(int n_frames, int frame_shift, int* n_samples);
int WorldMi355MlsaPade(int order, double* row);
int WorldMi355MlsaNoise(int64_t n, double* out);
/* The batch's f0_lengths are the T and its y_lengths must be WorldMi355MlsaSamples of them.
 * pitch: DEVICE float[total_frames]; lowpass, highpass: HOST double[n_low], double[n_high], uploaded by the library;
 * e: DEVICE double[total output samples] (WorldMi355BatchOutputOffsets); mc: DEVICE float[total_frames][order+1];
 * y: DEVICE double[total output samples]; status: DEVICE int[n_utt] or NULL: 0 fine; 1 a non-finite or negative pitch or a
 * non-finite coefficient: the utterance's samples are zeros (MlsaExcitation, which has no status, writes zeros too);
 * 2 a non-finite output sample: the samples are left as computed.  Utterances never exchange data.
 * MlsaSynthesis is MlsaExcitation and MlsaFilter in one call, bit for bit, without e in device memory beyond the block of
 * samples being filtered.
 * WM_ERR_BAD_ARG before any device call: T < 2, order outside 1 .. 62, pade_order outside 1 .. 7, |alpha| >= 1,
 * frame_shift < 1, n_low or n_high outside 1 .. 256, y_lengths that are not MlsaSamples of f0_lengths, a NULL pointer
 * (status excepted), a non-finite tap or pade entry.  Asynchronous on the context's stream.  Timed as "mlsa_kernel". */
int WorldMi355MlsaExcitation(WorldMi355Batch* b, const float* pitch, const double* lowpass, int n_low,
                             const double* highpass, int n_high, const WorldMi355MlsaOption* opt, double* e);
int WorldMi355MlsaFilter(WorldMi355Batch* b, const double* e, const float* mc, const WorldMi355MlsaOption* opt, double* y,
                         int* status);
int WorldMi355MlsaSynthesis(WorldMi355Batch* b, const float* pitch, const float* mc, const double* lowpass, int n_low,
                            const double* highpass, int n_high, const WorldMi355MlsaOption* opt, double* y, int* status);

/* ---- Objective evaluation: alignment by dynamic time warping and the distortion measures along a path ----
 * What tells a generated feature file from the natural one: mel-cepstral distortion in dB, the lf0 error on the frames both
 * sides call voiced, the voiced/unvoiced error, the distortion of any other stream.  The reference tree holds no evaluation
 * code.  PARITY IS UNPINNED: the yardstick is the definition below, which tests/dtw_reference.py states in numpy.
 * For utterance u, sequence A is the rows of `a` on the batch's frame layout: T_a is the batch's frame count of u, row t at
 * a + (frame_off[u] + t) * ld_a.  Sequence B is the rows of `b`: b_off is HOST int64[n_utt + 1], T_b = b_off[u+1] - b_off[u],
 * row t at b + (b_off[u] + t) * ld_b.  a and b are DEVICE float32.  Only the columns [first, first + count) of both enter.
 * Everything is computed in double:
 *   d(i, j) = sqrt( sum_{k = first .. first+count-1} (a[i][k] - b[j][k])^2 )        ascending k
 *   D(0,0) = d(0,0);  D(i,0) = d(i,0) + D(i-1,0);  D(0,j) = d(0,j) + D(0,j-1)
 *   D(i,j) = d(i,j) + min( D(i-1,j-1), D(i-1,j), D(i,j-1) )
 *   path:  backwards from (T_a-1, T_b-1) to (0,0); at (i,j) with i, j > 0 the predecessor with the smallest D,
 *          on equality (i-1,j-1) before (i-1,j) before (i,j-1); written in forward order
 * path: DEVICE int32[sum_u (T_a + T_b - 1)][2], pairs (i, j); utterance u starts at pair index frame_off[u] + b_off[u] - u
 * and its unused capacity is written (-1, -1).  path_len: DEVICE int32[n_utt].  cost: DEVICE double[n_utt], D(T_a-1, T_b-1).
 * status: DEVICE int[n_utt] or NULL.  Bit 1: a non-finite value in the used columns of either sequence; path_len is 0 and
 * cost NaN.  Bit 2: T_a = 0 or T_b = 0; path_len is 0 and cost 0.  A flagged utterance affects no other, and an utterance's
 * bits do not depend on the batch around it.
 * Limits: count 1 .. 64; T_a, T_b <= 32767.  WM_ERR_BAD_ARG before any device call: a limit exceeded, a NULL pointer (status
 * excepted), first < 0, first + count beyond ld_a or ld_b, a b_off that decreases or does not start at 0.  Asynchronous on
 * the context's stream.  Timed as "dtw_kernel" (the recurrence) and "dtw_path_kernel" (the walk).
 * The call keeps one byte per cell on the device (the back-pointers, in strips of 64 rows of A by T_b + 63 steps) and two
 * rows of D per pair, as the batch's workspace: DtwWorkspaceBytes says how much for these lengths (host only, no device
 * needed; WM_ERR_BAD_ARG for a NULL pointer or a length outside 0 .. 32767).  The descriptors of the pairs are kept with
 * b_off: a call with another b_off on the same batch waits for the stream and rebuilds them. */
int WorldMi355DtwWorkspaceBytes(int n_utt, const int* a_lengths, const int* b_lengths, int64_t* bytes);
int WorldMi355DtwAlign(WorldMi355Batch* b, const float* a, int64_t ld_a, const float* bs, int64_t ld_b, const int64_t* b_off,
                       int first, int count, int* path, int* path_len, double* cost, int* status);
/* The measures along a path.  path, path_len: DtwAlign's, or both NULL: the pairs are (k, k) for k < min(T_a, T_b), i.e.
 * truncation.  b_off as above.  b_mask: NULL or DEVICE uint8[b_off[n_utt]]; a pair whose B frame has mask 0 is left out (the
 * silences of the natural utterance's labels).  A pair outside [0, T_a) x [0, T_b) is left out too.  groups: HOST, 1 .. 8 of
 * them, rows of a and b laid out as above, each scored over its columns [first, first + count):
 *   kind 0, cepstral, in dB   e = (10 / ln 10) sqrt(2 sum_k D_k^2), D_k = a[i][k] - b[j][k], per counted pair
 *                             out: sum e, sum e^2, counted pairs, 0
 *   kind 1, log f0, count 1   a value above voiced_above is voiced; D = a - b in natural-log units
 *                             out: sum D^2 over the pairs voiced on both sides, the number of those pairs, the pairs whose
 *                             voicing differs, counted pairs
 * out: DEVICE double[n_utt][n_groups][4].  Sums run in pair order, in double; a left-out pair adds 0, so the order depends on
 * path_len alone.  An utterance DtwAlign flagged (path_len 0) gives zeros.
 * WM_ERR_BAD_ARG before any device call: as above, and n_groups outside 1 .. 8, a kind other than 0 and 1, kind 1 with count
 * other than 1, only one of path and path_len, a non-finite voiced_above.  Asynchronous on the context's stream. */
typedef struct {
  const float* a;
  int64_t ld_a;
  const float* b;
  int64_t ld_b;
  int first;
  int count;
  int kind;
} WorldMi355DistortionGroup;
typedef struct {
  double voiced_above;    /* -1e9: the recipe's unvoiced value is -1e10 */
} WorldMi355DistortionOption;
void WorldMi355DefaultDistortionOption(WorldMi355DistortionOption* opt);
int WorldMi355FeatureDistortion(WorldMi355Batch* b, const int* path, const int* path_len, const int64_t* b_off,
                                const unsigned char* b_mask, int n_groups, const WorldMi355DistortionGroup* groups,
                                const WorldMi355DistortionOption* opt, double* out);

/* ---- `cmp` composition (data/scripts/window.pl:45-146, addhtkheader.pl:45-82), SURVEY.md section 8(f) rank 3 ----
 * Applies each stream's dynamic-feature windows and lays the results side by side per frame:
 *   out[frame] = [stream 0: window 0 (dim) | window 1 | ...][stream 1: ...]...      (float32)
 * streams[s]: device pointer, float32 [total_frames][dims[s]].  windows[s][i]: HOST pointer to the
 * window_sizes[s][i] coefficients of window i of stream s (the content of data/win/NAME.win<i> without the
 * leading size).  Frames are clamped per utterance; -1e10 is the ignore value of unvoiced lf0.
 * Limits: 4 streams, 4 windows per stream, odd window sizes up to 15. */
int WorldMi355ComposeCmp(WorldMi355Batch* b, int n_streams, const float* const* streams, const int* dims,
                         const int* n_windows, const double* const* const* windows,
                         const int* const* window_sizes, float* out);

/* ---- Parameter generation: SPTK `mlpg` as gen_param drives it (scripts/Training.pl:2755-2810), the inverse of
 * WorldMi355ComposeCmp and the stage between a model's `cmp`-layout rows and WorldMi355RecipeDecode /
 * WorldMi355MelCepstrumToSpectrum.  One column is one utterance, one stream and one dimension, with T frames and the
 * stream's windows w_0 .. w_{n-1} (odd sizes, centre tap h_i = (size_i - 1) / 2):
 *   W  is the (n T) x T matrix whose row (t, i) holds w_i[k] at column t + k - h_i,
 *   mu the n T means, P the diagonal matrix of precisions 1 / variance,
 *   out the c that solves (W' P W) c = W' P mu     (banded LDL' in double; float32 in and out).
 * Columns never exchange data, utterances never exchange data. */
typedef struct {
  int edge;               /* 0 taps beyond the utterance dropped (SPTK mlpg); 1 clamped (window.pl, inverse of ComposeCmp) */
  int var_per_frame;      /* 0: var[s] is ONE row, used for every frame (gen_param's global variance, :2788-2791); 1: a row per frame */
  int input_type;         /* 0 variances, 1 precisions (mlpg -i 0 / -i 1) */
  double unvoiced_value;  /* written to every dim of an unvoiced frame of a stream with msd; default -1e10 */
} WorldMi355MlpgOption;
void WorldMi355DefaultMlpgOption(WorldMi355MlpgOption* opt);   /* 0, 0, 0, -1e10 */
/* mean[s]: DEVICE, row t of the batch at mean[s] + t * ld_mean: n_windows[s] * dims[s] floats laid
 *   [window 0: dim | window 1: dim | ...] as ComposeCmp writes a stream; var[s] the same layout with ld_var (ld_var is
 *   ignored and var[s] is one row when var_per_frame == 0).  One row stride for all streams: the call reads
 *   ComposeCmp's out (pointers into it, ld_mean = its columns) or an `ffo` row (:2778-2787) as it is.
 * dims, n_windows, windows, window_sizes: HOST, exactly as ComposeCmp.
 * msd: NULL, or per stream NULL or DEVICE: the stream's voicing value of frame t at msd[s] + t * ld_mean.  A frame is
 *   voiced when the value is >= 0.5 (:2782).  The solve runs over the whole utterance whatever the voicing, as gen_param
 *   does; afterwards every dim of an unvoiced frame holds unvoiced_value (0 gives the lf0 RecipeDecode expects).
 * out[s]: DEVICE float32 [total_frames][dims[s]], contiguous: what RecipeDecode takes.
 * status: DEVICE int[n_utt] or NULL, a bit mask per utterance: 1 a column holds a non-finite mean or variance, a
 *   variance <= 0, or with input_type 1 a precision < 0 (precision 0, an ignored observation, is allowed); 2 a pivot of
 *   the factorisation <= 0 or non-finite in a column with valid input: W' P W is not positive definite (no static
 *   window, singular ends).  A flagged column is zeros in every frame, whatever the voicing; no other column and no
 *   other utterance is affected.
 * Limits as ComposeCmp: 1-4 streams, 1-4 windows, odd sizes up to 15, dims >= 1.  A limit exceeded, a NULL required
 * pointer, ld_mean (ld_var with var_per_frame) smaller than a stream's row, edge or input_type out of range:
 * WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's stream; a batch of zero frames returns WM_OK. */
int WorldMi355ParameterGeneration(WorldMi355Batch* b, int n_streams, const float* const* mean, int64_t ld_mean,
                                  const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                                  const double* const* const* windows, const int* const* window_sizes,
                                  const float* const* msd, const WorldMi355MlpgOption* opt, float* const* out,
                                  int* status);
/* ---- Parameter generation considering global variance (GV): what HMGenS does with USEHMMGV = 1 and OPTKIND = NEWTON
 * (scripts/Training.pl:1892-1903), as a stage in ParameterGeneration's place; gen_wave then skips the postfilter
 * (:749-757).  Parity with HTS is unpinned: the yardstick is this definition (tests/gv_reference.py states it in numpy).
 * A column is one utterance, one stream and one dimension, with T frames and n windows; R = W' P W and r = W' P mu are
 * ParameterGeneration's, edge, var_per_frame and input_type included.  A frame is in the GV set G when it is voiced (a
 * stream with msd: value >= 0.5) and gv_mask, if given, is non-zero there; N = |G|.  Everything below is in double.
 *   start      c = ParameterGeneration's float32 output of the column, before its voicing overwrite
 *   moments    m = sum_{t in G} c_t / N,  e_t = c_t - m for t in G, else 0,  v = sum e_t^2 / N   (two passes)
 *   objective  f(c) = hmm_weight w (-1/2 c'Rc + c'r) - 1/2 gv_weight p_v (v - mu_v)^2,
 *              w = 1 / (n T), mu_v = gv_mean, p_v = 1 / gv_var
 *   scaling    with scale != 0, once before the loop: c_t <- m + sqrt(mu_v / v) e_t for t in G
 *   direction  g_t = hmm_weight w (r - Rc)_t - gv_weight p_v (v - mu_v) (2 / N) e_t
 *              H_t = -hmm_weight w R_tt - [t in G] gv_weight (2 / N^2) p_v ((N - 1)(v - mu_v) + 2 e_t^2)
 *              d_t = g_t / max(-H_t, 1e-3 hmm_weight w R_tt)        (the diagonal Newton step hts_engine publishes)
 *   loop       step = step_init; for trial 1 .. max_iter: c' = c + step d, d the direction at the current c;
 *              f(c') >= f(c): accept, step *= step_inc, and stop when epsilon > 0 and (f(c') - f(c)) / |f(c')| < epsilon;
 *              otherwise keep c and step *= step_dec
 *   output     float32(c), then unvoiced_value in the unvoiced frames as ParameterGeneration.
 * max_iter 0 with scale 0 is ParameterGeneration bit for bit.  Columns and utterances never exchange data, and the sums
 * are taken in an order that depends on T alone: an utterance's bits do not depend on the batch around it. */
typedef struct {
  int max_iter;           /* trials, accepted or not (MAXGVITER); default 50 */
  int scale;              /* 1: start from the trajectory scaled to the GV mean; default 1 */
  double epsilon;         /* relative gain below which an accepted trial ends the loop (GVEPSILON); 0 never; default 1e-4 */
  double step_init;       /* STEPINIT 1 */
  double step_inc;        /* STEPINC 1.2 */
  double step_dec;        /* STEPDEC 0.5 */
  double hmm_weight;      /* HMMWEIGHT 1 */
  double gv_weight;       /* GVWEIGHT 1 */
} WorldMi355GvOption;
void WorldMi355DefaultGvOption(WorldMi355GvOption* opt);       /* 50, 1, 1e-4, 1, 1.2, 0.5, 1, 1 */
/* ParameterGeneration's arguments (opt is its option; msd, out and status as there) and
 * gv_mean[s], gv_var[s]: DEVICE float32 [dims[s]]: the mean and the variance of the per-utterance variance (gv.mean,
 *   gv.var restricted to the stream's statics).
 * gv_mask: NULL, or DEVICE uint8 [total_frames]: 0 takes a frame out of G in every stream (silence: NOSILGV).
 * info: NULL, or DEVICE double [n_utt][sum of dims][4]: f at the start of the loop, f at its end, trials, accepted
 *   trials; zeros for a column that is returned as ParameterGeneration leaves it.
 * status: ParameterGeneration's bits 1 and 2 (such a column stays zeros); further 1: a gv_mean or gv_var of the column
 *   that is not positive and finite; 4: N < 2, or v not positive and finite at the start.  A column with 1 or 4 is
 *   ParameterGeneration's, with the voicing overwrite; no other column is affected.
 * WM_ERR_BAD_ARG before any device call: what ParameterGeneration refuses; a NULL gv_mean, gv_var, gv or entry of
 * them; max_iter < 0 or above 100000; scale not 0 or 1; epsilon negative or non-finite; a step_init, step_inc, step_dec
 * or hmm_weight that is not positive and finite; a gv_weight negative or non-finite.
 * Asynchronous on the context's stream; a batch of zero frames returns WM_OK.  Timed as "mlpg_kernel" (the start) and
 * "mlpg_gv_kernel". */
int WorldMi355ParameterGenerationGv(WorldMi355Batch* b, int n_streams, const float* const* mean, int64_t ld_mean,
                                    const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                                    const double* const* const* windows, const int* const* window_sizes,
                                    const float* const* msd, const WorldMi355MlpgOption* opt,
                                    const float* const* gv_mean, const float* const* gv_var,
                                    const unsigned char* gv_mask, const WorldMi355GvOption* gv, float* const* out,
                                    double* info, int* status);
/* ---- Trajectory training criterion with gradients: DNNDefine.trajectory_cost (data/scripts/DNNDefine.py:240-399) as
 * DNNTraining.py -w win drives it (scripts/Training.pl:930-940), for a whole batch of utterances.  Rows are in the `ffo`
 * layout (per stream an optional voicing column, then [window 0: dim | window 1: dim | ...]); per column (utterance,
 * stream, dimension) of T frames with the stream's windows, W_i as ParameterGeneration's W at edge 0 for window i alone:
 *   A = sum_i p_i W_i' W_i,  c = A^-1 sum_i p_i W_i' mu_i,  e = o - c  (o the observed static),  p_i = 1 / var_i,
 *   trj = (D T ln 2pi - sum_d ln det A_d + sum_d e_d' A_d e_d) / (2 D T),
 *   msd = (M T ln 2pi + T sum_m ln var_m + sum_m sum_t (pred_m - obs_m)^2 / var_m) / (2 M T)     (0 when M = 0),
 *   gv  = (D ln 2pi + sum_d ln gv_var_d + sum_d (pv_d - ov_d)^2 / gv_var_d) / (2 D),  pv, ov the variances over t of c, o,
 *   utterance cost = trj + msd_weight msd + gv_weight gv,
 * D the sum of dims, M the number of streams with a voicing column.  A is banded: the factor, ln det A, the band of
 * A^-1 that the variance gradient needs and both solves cost O(T) per column, in double (float32 in).  Utterances never
 * exchange data: an utterance's bits do not depend on the batch around it. */
typedef struct {
  int edge;               /* 0: taps beyond the utterance dropped, the reference's window matrix; nothing else is accepted */
  double msd_weight;      /* default 1 */
  double gv_weight;       /* default 1e-6 */
} WorldMi355TrajectoryOption;
void WorldMi355DefaultTrajectoryOption(WorldMi355TrajectoryOption* opt);   /* 0, 1, 1e-6 */
/* pred[s], obs[s]: DEVICE, the stream's window 0 of row t at pred[s] + t * ld (n_windows[s] * dims[s] floats), as
 *   ParameterGeneration's mean; of obs only the static window is read.  var[s]: DEVICE, ONE row of
 *   n_windows[s] * dims[s] variances.  gv_var[s]: DEVICE, dims[s] variances of the per-utterance variance.
 * dims, n_windows, windows, window_sizes: HOST, as ComposeCmp; window sizes 1, 3 or 5.
 * msd_pred, msd_obs, msd_var: NULL (no stream has a voicing column), or per stream NULL or DEVICE: the voicing column
 *   of row t at msd_pred[s] + t * ld, msd_obs[s] + t * ld, and its one variance at msd_var[s].
 * cost: DEVICE double [n_utt][3]: trj, msd, gv.
 * c: NULL, or per stream DEVICE float32 [total_frames][dims[s]], contiguous.
 * grad_pred: NULL, or per stream DEVICE: the gradient of the utterance's cost with respect to pred, at
 *   grad_pred[s] + t * ld_grad; grad_msd: NULL, or per stream NULL or DEVICE, the voicing column's, same stride.
 * grad_var: NULL, or DEVICE double [n_utt][width], the gradient of each utterance's cost with respect to the variance
 *   row in the `ffo` layout of the streams as given (width = sum_s [voicing column] + n_windows[s] * dims[s]).
 * status: NULL, or DEVICE int[n_utt], a bit mask: 1 a non-finite pred or obs, or a variance (gv_var and the voicing
 *   column's included) that is not positive and finite; 2 a pivot <= 0 (no static window).  A flagged utterance has
 *   costs 0 and gradients 0, and c is zeros in the flagged columns; other utterances keep their bits.
 * A count out of range (1-4 streams, 1-4 windows, dims >= 1), a NULL required pointer, ld (ld_grad with grad_pred
 * or grad_msd) smaller than a stream's row, edge != 0, a window size even or above 5: WM_ERR_BAD_ARG before any device call.
 * Asynchronous on the context's stream; a batch of zero frames returns WM_OK.  Timed as "trj_kernel". */
int WorldMi355TrajectoryCost(WorldMi355Batch* b, int n_streams, const float* const* pred, const float* const* obs,
                             int64_t ld, const float* const* var, const float* const* gv_var, const int* dims,
                             const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                             const float* const* msd_pred, const float* const* msd_obs, const float* const* msd_var,
                             const WorldMi355TrajectoryOption* opt, double* cost, float* const* c,
                             float* const* grad_pred, float* const* grad_msd, int64_t ld_grad, double* grad_var,
                             int* status);
/* ---- Acoustic model forward pass: DNNDefine.inference (data/scripts/DNNDefine.py:113-191) as DNNSynthesis.py:129-229
 * runs it (keep_prob 1), with the frame-level DNNDefine.cost (:231-237), for a whole batch of utterances: `.ffi` rows in,
 * `ffo`-layout means out.  Per frame of utterance u with speaker s(u), float32, every addition rounded in this order:
 *   h_{i+1} = act_h((h_i W_i + b_i) + sd_i[s(u)])   (the speaker row only with spkr_weights),   out = act_o(h_L W_o + b_o);
 * a product h W is a k-ordered fmaf chain from zero (the exact-f32 matrix instruction).  With n_layers = 0 the inputs
 * feed the output layer.  Cost per utterance of T frames, D = n_outputs, var = variances[s(u)], in double:
 *   cost = (ln 2pi + (1 / D) sum_d ln var_d + (1 / (T D)) sum_t sum_d (obs - out)^2 / var_d) / 2.
 * A row's result depends on that row of x and on the model alone: not on the chunking, not on the batch around it. */
typedef struct {
  int n_layers, n_inputs, n_outputs, n_spkrs;    /* n_layers 0 .. 8; n_spkrs >= 1 */
  int hidden_activation, output_activation;      /* 0 linear, 1 sigmoid, 2 tanh, 3 relu (Config.pm.in:228) */
  const int* units;                              /* HOST [n_layers] */
  const float* const* weights;                   /* HOST array of n_layers + 1 DEVICE pointers, [fan_in][fan_out] */
  const float* const* biases;                    /* likewise, [fan_out] */
  const float* const* spkr_weights;              /* NULL (SD), or n_layers DEVICE pointers [n_spkrs][units[i]] */
  const float* variances;                        /* DEVICE [n_spkrs][n_outputs], or NULL when no cost is asked */
  int64_t max_chunk_frames;                      /* frames that go through the layers together; 0: 65 536; at most 2^20 */
} WorldMi355AcousticModel;
/* x: DEVICE, row t at x + t * ld_x (n_inputs floats).  spkr: HOST [n_utt], or NULL: n_spkrs - 1 for every utterance
 *   (DNNSynthesis.py:139).  out: DEVICE, row t at out + t * ld_out (n_outputs floats).  obs: DEVICE, the targets, row t
 *   at obs + t * ld_obs; read only with cost.  cost: NULL, or DEVICE double [n_utt].
 * status: NULL, or DEVICE int[n_utt], a bit mask: 1 a non-finite value in the utterance's rows of x (of obs too when a
 *   cost is asked); 2 a non-finite output of finite inputs, or, when a cost is asked, a variance of its speaker that is
 *   not positive and finite.  A flagged utterance has zero rows in out and cost 0; other utterances keep their bits.
 * A NULL required pointer, a count out of range (n_layers outside 0 .. 8, a unit count, n_inputs, n_outputs or n_spkrs
 * below 1, max_chunk_frames below 0), an activation code outside 0 .. 3, a speaker index outside [0, n_spkrs), a leading
 * dimension smaller than its row, cost without obs or without variances, a layer so wide that a chunk's 128 x 128 tiles
 * exceed 2^31 - 1: WM_ERR_BAD_ARG before any device call.
 * The hidden activations live in the batch's workspace (two [chunk][max units] float32 buffers, kept between calls).
 * Asynchronous on the context's stream; a batch of zero frames returns WM_OK.  Timed as "dnn_layer_kernel" (the input
 * check and all layers of a call as one record) and "dnn_cost_kernel". */
int WorldMi355AcousticModelForward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const float* x, int64_t ld_x,
                                   const int* spkr, float* out, int64_t ld_out, const float* obs, int64_t ld_obs,
                                   double* cost, int* status);
/* ---- Acoustic model training pass: DNNTraining.py's step on the network above -- the forward pass with dropout
 * (DNNDefine.inference at keep_prob < 1, TF 1.x tf.nn.dropout), the gradients of the frame-level cost, and the backward
 * pass through the network.  Hidden layer i, batch row t (0 .. total_frames - 1), unit n:
 *   mask m = 1 iff (float)(w >> 8) * 2^-24 < keep_prob, w word n & 3 of Philox4x32-10 (multipliers 0xD2511F53,
 *   0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) at counter (t, n >> 2, i, offset), key (seed & 0xffffffff,
 *   seed >> 32): a function of (seed, offset, i, t, n) alone;
 *   a_i = act_h((h_{i-1} W_i + b_i) + sd_i[s(u)]),  h_i = m ? fl(a_i / keep_prob) : 0  (h_i = a_i at keep_prob 1),
 *   out = act_o(h_{L-1} W_o + b_o): no dropout on the outputs.  With keep_prob 1 out equals AcousticModelForward's bits.
 * Backward from G = dloss/dout:  dz_o = G act_o'(out),  dh_{i-1} = dz_i W_i',  da_i = m ? fl(dh_i / keep_prob) : 0,
 *   dz_i = da_i act_h'(a_i)  (the derivative from the float32 a: a (1 - a), 1 - a^2, [a > 0], 1),
 *   dW_i[k][n] = sum_t h_{i-1}[t][k] dz_i[t][n]: one k-ordered float32 fmaf chain over the batch's rows in order,
 *   db_i = sum_t dz_i,  dsd_i[s] = the same over the rows of speaker s: both in double, utterance by utterance in a fixed
 *   order that depends on the lengths alone, rounded once.  No result depends on max_chunk_frames.
 * Cost gradients per utterance of T frames (D = n_outputs, var = variances[s(u)]), in double:
 *   grad_out[t][d] = (out - obs) / (var_d T D)  (rounded to float32),
 *   grad_var[u][d] = (1 / var_d - (1 / T) sum_t (obs - out)^2 / var_d^2) / (2 D). */
typedef struct {
  float keep_prob;        /* 0 < keep_prob <= 1 */
  uint64_t seed;
  uint32_t offset;        /* the caller's step counter */
} WorldMi355Dropout;
/* AcousticModelForward's arguments, and: drop: HOST, NULL for keep_prob 1.  grad_out: NULL, or DEVICE float32, row t at
 *   grad_out + t * ld_grad.  grad_var: NULL, or DEVICE double [n_utt][n_outputs].  Either asks for obs and variances, as a
 *   cost does.  status as AcousticModelForward's; a flagged utterance has zero rows in out and grad_out, a zero row in
 *   grad_var and cost 0.  Refusals as AcousticModelForward's, and: keep_prob outside (0, 1] or not finite, ld_grad smaller
 *   than a row.  Timed as "dnn_layer_kernel" and "dnn_cost_kernel". */
int WorldMi355AcousticModelTrainForward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop,
                                        const float* x, int64_t ld_x, const int* spkr, float* out, int64_t ld_out,
                                        const float* obs, int64_t ld_obs, double* cost, float* grad_out, int64_t ld_grad,
                                        double* grad_var, int* status);
/* The backward pass: the forward pass is computed again from x with the same mask.  grad_out: DEVICE, G, row t at
 *   grad_out + t * ld_grad.  grad_weights, grad_biases: NULL, or HOST arrays of n_layers + 1 DEVICE pointers shaped as
 *   the model's; grad_spkr_weights: NULL, or n_layers DEVICE pointers [n_spkrs][units[i]] (refused without
 *   spkr_weights).  The gradients are overwritten.  status: NULL, or DEVICE int[n_utt]: 1 a non-finite value in the
 *   utterance's rows of x or of G; 2 a non-finite output of finite inputs.  A flagged utterance adds exact zeros to every
 *   gradient; the others' contributions keep their bits.  Refusals as above, and a NULL entry in a given pointer array.
 * A batch of zero frames returns WM_OK with zero gradients.  The workspace (per chunk row: two dz buffers and, per hidden
 * layer, a_i and with keep_prob < 1 also h_i, each max(units, n_outputs) floats) is the forward pass's, grown.  Timed as
 * "dnn_backward_kernel", one record per call. */
int WorldMi355AcousticModelBackward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop,
                                    const float* x, int64_t ld_x, const int* spkr, const float* grad_out, int64_t ld_grad,
                                    float* const* grad_weights, float* const* grad_biases, float* const* grad_spkr_weights,
                                    int* status);
/* ---- The optimisers' update step: DNNDefine.get_optimizer (data/scripts/DNNDefine.py:65-80) names six tf.train.*
 * optimisers of TF 1.x, which DNNDefine.training (:194-213) applies to three groups of tensors at three rates.  One call
 * updates every tensor of every group in ONE launch.  rule: 0 sgd, 1 momentum, 2 adagrad, 3 adadelta, 4 adam, 5 rmsprop.
 * With g the gradient, p the parameter, r the tensor's rate -- everything float32, every operation rounded on its own in
 * the order written, nothing contracted into a fused multiply-add, division and square root correctly rounded,
 * subnormals kept; 1 - rho and 1 - beta are float32 differences of the float32 fields:
 *   rule                                 slots (initial value)  update
 *   sgd                                  -                      p <- p - r g
 *   momentum (momentum 0.9)              a (0)                  a <- a mu + g;  p <- p - a r
 *   adagrad                              a (0.1)                a <- a + g g;  p <- p - (g r) / sqrt(a)
 *   adadelta (rho 0.95, epsilon 1e-8)    a (0), b (0)           a <- a rho + (g g) (1 - rho);
 *                                                               u = (sqrt(b + eps) / sqrt(a + eps)) g;  p <- p - u r;
 *                                                               b <- b rho + (u u) (1 - rho)
 *   adam (beta 0.9, 0.999, epsilon 1e-8) m (0), v (0)           alpha = r sqrt(1 - beta2_power) / (1 - beta1_power), on
 *                                                               the host in float32;  m <- m + (g - m) (1 - beta1);
 *                                                               v <- v + (g g - v) (1 - beta2);
 *                                                               p <- p - (m alpha) / (sqrt(v) + eps)
 *   rmsprop (rho 0.9, epsilon 1e-10)     s (1)                  s <- s + (g g - s) (1 - rho);
 *                                                               p <- p - (g r) / sqrt(s + eps)
 * The slots are the caller's, and so are their initial values (slot0: a, m, s; slot1: b, v).  beta1_power and beta2_power
 * are TF's variables of that name: they start at beta1 and beta2, and the CALLER multiplies them by beta1 and beta2 after
 * each step.  RMSprop is TF's at momentum 0, whose `momentum` slot holds the last update alone: it is not kept.  A rate of
 * 0 is a rate: the slots move and p keeps its bits. */
typedef struct { int rule; float momentum, rho, beta1, beta2, epsilon, beta1_power, beta2_power; } WorldMi355OptimizerOption;
/* TF 1.x's defaults for `rule` (the table above); the powers are the betas. */
void WorldMi355DefaultOptimizerOption(int rule, WorldMi355OptimizerOption* opt);
/* param, grad, slot0, slot1: HOST arrays [n_tensors] of DEVICE float32 pointers, tensor k holding count[k] contiguous
 * elements; count, rate: HOST [n_tensors].  slot0 is needed by every rule but sgd, slot1 by adadelta and adam; an array
 * the rule does not need may be NULL and is not read.  Elements move 16 bytes at a time where all pointers of a tensor
 * are 16-byte aligned, else one by one: the same bits either way.  status: NULL, or DEVICE int[n_tensors], zeroed by the
 * call: 1 where a gradient element of the tensor is not finite; the update is applied as written all the same, as TF
 * does.  n_tensors outside 1 .. 64, a rule outside 0 .. 5, a NULL required array or entry, a count below 1, a rate that
 * is negative or not finite, a field of opt that is not finite, for adam a power outside (0, 1): WM_ERR_BAD_ARG before
 * any device call.  A call of the context, not of a batch; asynchronous on the context's stream. */
int WorldMi355OptimizerStep(WorldMi355Context* ctx, const WorldMi355OptimizerOption* opt, int n_tensors,
                            float* const* param, const float* const* grad, float* const* slot0, float* const* slot1,
                            const int64_t* count, const float* rate, int* status);
/* ---- Mel-cepstral postfilter: the recipe's formant emphasis, postfiltering_mcp (scripts/Training.pl:2642-2687), which
 * gen_wave (:2813-2845) runs on every generated `.mgc` before mgc2sp -- the stage between
 * WorldMi355ParameterGeneration and WorldMi355MelCepstrumToSpectrum.  For one frame c[0 .. order] at warp alpha and
 * w = [1, 1, beta, ..., beta] (:2646-2651):
 *   out[0] = c[0] + delta,   out[k] = w[k] c[k] (k >= 1),   delta = 1/2 ln(E(c) / E(w c)),
 * E(v) being `freqt -m order -a alpha -M co -A 0 | c2acr -m co -M 0 -l length` of v (:2654-2662): the mean over the
 * `length` bins of the power spectrum of v.  mc2b, the addition to b[0] and b2mc (:2664-2682) amount to the first line.
 * E is evaluated in double at the script's bins in the limit co -> infinity, directly at the warped frequencies; the
 * script's co = 2047 leaves out at most twice sum_{n > co} |freqt(w c)[n]| (5e-431 at order 49, alpha 0.55), far
 * below the float32 rounding of its intermediate files (1e-7).  Fields: alpha the `mgc` stream's warp ($fw), beta $pf_mcp
 * (config default 1.4), order m, length $fl = IMPLEN (4096), independent of the batch's fft_size.  hts_engine's -b
 * postfilter (:810) is not offered; the LSP postfilter (:2690-2752) is WorldMi355LspPostfilter above; the
 * modulation-spectrum postfilter (:2950), which gen_wave runs INSTEAD of this one with USEMSPF, is
 * WorldMi355ModulationSpectrumPostfilter below. */
typedef struct {
  double alpha;
  double beta;
  int order;
  int length;
} WorldMi355McpfOption;
/* alpha 0.35, beta 1.4, order 25, length 4096. */
void WorldMi355DefaultMcpfOption(WorldMi355McpfOption* opt);
/* mc, out: DEVICE double[total_frames][order+1]; out == mc (in place) is allowed.  gain: DEVICE double[total_frames] or
 * NULL: delta.  out[0] is exactly the rounded sum c[0] + delta with that delta, out[k] exactly the one product
 * w[k] c[k]; c[0] does not enter delta.  status: DEVICE int[total_frames] or NULL: 0 fine, 1 a non-finite coefficient,
 * 2 a sum that is not finite and positive (exp overflowed); such rows are zeros with gain 0.  Frames never exchange
 * data.  beta == 1 or order == 1 is the identity (gen_wave skips the step at 1.0, :2838): rows copied bit for bit,
 * gain 0, status 0, no energy computed.  A NULL mc, opt or out, order outside 1 .. 63, not |alpha| < 1, a non-finite
 * beta, length not a power of two in 64 .. 8192: WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's
 * stream; a batch of zero frames returns WM_OK. */
int WorldMi355MelCepstrumPostfilter(WorldMi355Batch* b, const double* mc, const WorldMi355McpfOption* opt, double* out,
                                    double* gain, int* status);
/* ---- Parameter modification: F0 scaling and formant shift, ParameterModification of the reference's own example
 * (externs/WORLD_v2/test/test.cpp:201-238), the step between analysis and synthesis.  Per utterance u there are two
 * factors, shift = f0_scale[u] and ratio = formant_ratio[u]:
 *   f0_out[i] = f0[i] * shift: one product, an unvoiced 0 stays 0, nothing is clamped                      (:204-207)
 *   per frame, F = fft_size, n = F / 2 + 1, l[j] = log(sp[j]):                                             (:211-227)
 *     knots x1[j] = ratio * j / F * fs (left to right, in double), queries x2[i] = (double)i / F * fs,
 *     out[i] = exp(interp1(x1, l, n, x2, n)[i]), interp1 being src/matlabfunctions.cpp:157-182 (histc :136-155):
 *     k = clamp(#{j : x1[j] <= x2[i]}, 1, n - 1), s = (x2[i] - x1[k-1]) / (x1[k] - x1[k-1]), l[k-1] + s (l[k] - l[k-1])
 *   if ratio < 1, c = int(F / 2.0 * ratio): out[j] = out[c - 1] for j = c .. F / 2                         (:228-232)
 * k and s are the reference's, ties (s == 0) included, so non-finite values land where the reference puts them: a zero
 * bin has l = -inf and finite + 0 * (-inf) is NaN (ratio 1.0: a zero at bin i gives NaN at i - 1 and i).  Nothing is
 * repaired.  A ratio of exactly 1.0 still goes through exp(log(.)); only a NULL factor array skips its part.  The
 * aperiodicity is not touched, as in the reference.
 * f0_scale, formant_ratio: HOST double[n_utt], or NULL: that part is not done and its pointers are not read.
 * f0, f0_out: DEVICE double[total_frames]; sp, sp_out: DEVICE double[total_frames][fft_size/2+1]; f0_out == f0 and
 * sp_out == sp (in place) are allowed.  The factors are copied before the call returns.  WM_ERR_BAD_ARG before any
 * device call: both factor arrays NULL; a factor that is not finite or not > 0; ratio < 2.0 / F (the reference would
 * read out[-1]) or ratio > F; a NULL data pointer of a part that is asked for; an output that overlaps its input other
 * than exactly.  fft_size other than 512 .. 4096 with a ratio: WM_ERR_UNSUPPORTED_FFT.  Asynchronous on the context's
 * stream; a batch of zero frames returns WM_OK. */
int WorldMi355ModifyFeatures(WorldMi355Batch* b, const double* f0_scale, const double* formant_ratio, const double* f0,
                             const double* sp, double* f0_out, double* sp_out);
/* ---- Modulation-spectrum postfilter: postfiltering_mspf (scripts/Training.pl:2950-3000, msmp2seq :3003-3038), which
 * gen_wave runs on every generated `.mgc` INSTEAD of postfiltering_mcp when the recipe is configured with USEMSPF=1,
 * and the sums behind its statistics files (make_mspf, :3133-3221).  Settings: frame_length Lw ($mspfLength, odd),
 * fft_length N ($mspfFFTLen), emphasis e ($mspfe{'mgc'}); S = (Lw - 1) / 2, K = N / 2 + 1.  For one utterance of T >= 1
 * frames and one column x[0 .. T):
 *   1  mu = mean(x), y = x - mu                                                        (vstat -o 1, vopr -s)
 *   2  J = ceil((T + S) / S) frames, z_j[i] = w[i] y[j S - S + i], i < Lw, y = 0 outside [0, T), zeros up to N
 *   3  w = SPTK's Bartlett window (window -w 3 -n 0): 2 i / (Lw - 1) for i < Lw / 2, else 2 - 2 i / (Lw - 1)
 *   4  X_j = DFT_N(z_j), m_j[k] = 1/2 ln(|X_j[k]|^2 + 1e-30), k < K                    (spec -o 1 -e 1e-30)
 *   5  m' = m + e (((m - mean_gen[k]) / std_gen[k]) std_nat[k] + mean_nat[k] - m)       (:2973-2982)
 *   6  X'_j[k] = exp(m') X_j[k] / |X_j[k]| (exp(m') where X_j[k] = 0), v_j the N-point inverse real transform
 *   7  seq[j S + n] += v_j[n] for all n < N (the circular tail included), out[t] = seq[S + t] + mu
 * The statistics are the mean and the population standard deviation sqrt(E[m^2] - E[m]^2) of m per column and bin over
 * every frame of every sequence, the all-zero trailing frames included, as the script counts them.  Two things are
 * taken from SPTK's documented behaviour and were not confirmed against its binaries: the division by n in vstat's
 * variance and the frame count of `frame`.  The script rounds to float32 at every pipe and to about 6 digits at
 * `x2x +fa`; the library computes in double throughout (std_nat / std_gen is formed once per bin on the host).  A column
 * that is zero after its mean has bins whose phase is rounding noise, which a std_nat / std_gen below 1 lifts out of
 * the 1e-30 floor: there the script itself is unstable. */
typedef struct {
  int frame_length;
  int fft_length;
  double emphasis;
} WorldMi355MspfOption;
/* frame_length 25, fft_length 64, emphasis 1.0. */
void WorldMi355DefaultMspfOption(WorldMi355MspfOption* opt);
/* x, out: DEVICE double[total_frames][dim], out != x (a time segment reads its neighbours' input).  mean_gen, std_gen,
 * mean_nat, std_nat: HOST double[dim][K], validated here and uploaded to the batch's workspace.  status: DEVICE
 * int[n_utt] or NULL, a bit mask per utterance: 1 a column holds a non-finite input (or its mean overflows), 2 a result
 * is not finite (exp overflowed).  Such a column is zeros in every frame of that utterance; nothing else is affected.
 * A result depends on its own utterance and column alone: the same bits whatever the batch around it.  A NULL x, out
 * or table, dim < 1, fft_length outside {16, 32, 64}, frame_length even, below 3 or above fft_length - 1, a non-finite
 * emphasis or table entry, a std_gen entry <= 0, out == x: WM_ERR_BAD_ARG before any device call.  Asynchronous on the
 * context's stream; a batch of zero frames returns WM_OK, an utterance of zero frames contributes nothing. */
int WorldMi355ModulationSpectrumPostfilter(WorldMi355Batch* b, const double* x, int dim, const WorldMi355MspfOption* opt,
                                           const double* mean_gen, const double* std_gen, const double* mean_nat,
                                           const double* std_nat, double* out, int* status);
/* Steps 1-4 over the batch: sum, sumsq: DEVICE double[dim][K], overwritten with the sums of m and m^2 over every frame
 * of every utterance (per utterance in frame order, the utterances added in index order: no atomics, the same bits
 * every time).  mean: DEVICE double[n_utt][dim] or NULL; NULL takes each utterance's own column means, non-NULL serves
 * silence removal, where the mean is the whole utterance's and x holds the kept segments.  n_frames: HOST, receives the
 * sum of J over the utterances, at once.  The caller adds across batches and finalises: mean = sum / n,
 * std = sqrt(sumsq / n - mean^2).  Refusals as above. */
int WorldMi355ModulationSpectrumStats(WorldMi355Batch* b, const double* x, int dim, const WorldMi355MspfOption* opt,
                                      const double* mean, double* sum, double* sumsq, int64_t* n_frames);
/* mean: DEVICE double[n_utt][dim], the column means of x per utterance (zeros for an utterance of zero frames, NaN for
 * a column with a non-finite value), summed in a fixed order that depends on the utterance's length alone. */
int WorldMi355ColumnMeans(WorldMi355Batch* b, const double* x, int dim, double* mean);
/* The output frames one wave of the postfilter handles; longer utterances are cut into such segments, which does not
 * change a bit of the result. */
int WorldMi355MspfSegmentFrames(void);
/* ---- The stages after `cmp`: the recipe's `ffo` and `stats` targets (data/Makefile.in:325-459) and the data of GV
 * training (make_data_gv, scripts/Training.pl:1402-1491) rest on the three calls below.
 *
 * Gap interpolation, data/scripts/interpolate.pl:68-105.  x, out: DEVICE float32 [total_frames][dim], out != x.  A value
 * is a gap when it equals (float)ignore_value: -1e10 (exact in float32) is the script's own comparison; 0 and 1e-8 are
 * what this fork's analysis CLI and Extract.py leave in unvoiced frames.  Per utterance and column: a gap between the
 * valid frames lo < t < hi becomes (float)(a + step (t - lo)), a = (double)x[lo], step = ((double)x[hi] - a) / (hi - lo),
 * in double with the product and the sum rounded separately, which gives the script's bits; a leading gap takes the
 * first valid value, a trailing gap the last; valid frames are copied.  NaN is a valid value and propagates.
 * voiced: NULL, or DEVICE float32 [total_frames]: 1.0 where column 0 of x is valid, else 0.0 (`sopr -magic -1.0E+10
 * -m 0 -a 1 -MAGIC 0`, Makefile.in:347/:381).  status: NULL, or DEVICE int[n_utt]: bit 1 a column of the utterance holds
 * no valid value (the script dies with "no valid value"); that column is zeros in out, nothing else is affected.  An
 * utterance never reads another's frames; a result depends on its own utterance and column alone.  A NULL x or out,
 * dim < 1, out == x, a non-finite ignore_value: WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's
 * stream; a batch of zero frames returns WM_OK. */
int WorldMi355InterpolateGaps(WorldMi355Batch* b, const float* x, int dim, double ignore_value, float* out, float* voiced,
                              int* status);
/* An `ffo` row (Makefile.in:373-408): WorldMi355ComposeCmp's arguments and results, and msd: NULL, or per stream NULL
 * or DEVICE float32 [total_frames], which becomes ONE column in front of that stream's windows:
 *   out[frame] = [stream 0: msd, if any | window 0 (dim) | window 1 | ...][stream 1: ...]...
 * Limits as ComposeCmp; a limit exceeded or a NULL required pointer: WM_ERR_BAD_ARG before any device call. */
int WorldMi355ComposeFfo(WorldMi355Batch* b, int n_streams, const float* const* streams, const int* dims,
                         const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                         const float* const* msd, float* out);
/* Per-utterance column moments.  x: DEVICE float32, row t of the batch at x + t * ld, ld >= width: a column view of a
 * wider matrix works as it is.  ignore_value: HOST pointer or NULL; when given, a value equal to (float)*ignore_value is
 * left out of its own column (make_data_gv's `grep -v '1e+10'`, :1448, counted per column).  count, mean, m2: DEVICE
 * [n_utt][width]: the number of kept values, their mean, and the sum of (x - mean)^2 around that computed mean, both in
 * double -- two passes, not sum x^2.  A count of 0 gives mean 0 and m2 0.  Summed in a fixed order that depends on the
 * utterance's length alone (WorldMi355ColumnMeans' order): the same bits whatever the batch around the utterance, no
 * atomics.  width is taken 64 columns per block and has no limit of its own.  A NULL x, count, mean or m2, width < 1,
 * ld < width, a non-finite *ignore_value: WM_ERR_BAD_ARG before any device call.  Asynchronous on the context's stream;
 * a batch of zero frames returns WM_OK. */
int WorldMi355ColumnMoments(WorldMi355Batch* b, const float* x, int64_t ld, int width, const double* ignore_value,
                            int64_t* count, double* mean, double* m2);
/* ---- The acoustic model's input rows from aligned labels: data/scripts/makefeature.pl, which make_train_data_dnn and
 * make_gen_data_dnn (scripts/Training.pl:1677-1723) pipe every label file through; the result is the `.ffi` rows that
 * WorldMi355AcousticModelForward reads.
 *
 * A feature of the question config.  kind 0: binary, pattern is the text between the braces, comma-separated
 * alternatives; the feature is 1 when any alternative matches the whole label name.  kind 1: float, one alternative
 * with exactly one %d; the captured integer, normalised.  kind 2 .. 7: the reserved names in the order of
 * makefeature.pl:55 -- state in phone forward / backward, frame in state forward / backward, frame in phone forward /
 * backward; pattern is not read.  min, max: kinds 1 .. 7.  In a pattern `*` is any run of characters, `?` zero or ONE
 * character, `.` any one character (the script does not escape it), every other byte itself; the match is Perl's
 * ^...$ in backtracking order, which decides what %d ([+-]?[0-9]+) captures when several ways match.  A value below
 * min is 0, above max 1 (the script's "Out of range" warning), else (float)((double)(v - min) / (double)(max - min)):
 * the bits `perl makefeature.pl | x2x +af` gives for max - min <= 2^20.  An unmatched float feature is 0.
 * Refused when the set is made: a pattern byte outside 0x21-0x7E, one of \ ( ) { } in a pattern (the script leaves them
 * active as regex syntax), an alternative of more than 63 tokens (%d is one token): WM_ERR_UNSUPPORTED; a kind outside
 * 0 .. 7, a NULL pattern, a float pattern without exactly one %d or with a comma, max - min > 2^20, and max <= min:
 * WM_ERR_BAD_ARG -- this last differs from the script, which divides by zero only when it gets there.  An empty
 * alternative is valid and matches nothing.  A captured integer beyond the range of int saturates.
 * The float features are host work (a few dozen per config, evaluated once per distinct name of a call by a
 * backtracking matcher and uploaded as a float32 table); the binary features are the device's.
 * The set owns its device tables and is destroyed before its context. */
typedef struct { int kind; const char* pattern; int min, max; } WorldMi355LabelFeature;
typedef struct WorldMi355LabelFeatureSet WorldMi355LabelFeatureSet;
int WorldMi355CreateLabelFeatureSet(WorldMi355Context* ctx, int n_features, const WorldMi355LabelFeature* features,
                                    WorldMi355LabelFeatureSet** out);
void WorldMi355DestroyLabelFeatureSet(WorldMi355LabelFeatureSet* set);
int WorldMi355LabelFeatureCount(const WorldMi355LabelFeatureSet* set);
/* The rows of a batch (a synthesis-style one: f0_lengths only).  Utterance u owns the label lines line_off[u] ..
 * line_off[u+1]-1 (HOST, n_utt + 1 offsets); per line (HOST): start and end in frames (int(0.5 + time / frame_shift)),
 * state_index (the integer >= 2 in the name's trailing [..], else 0) and name, the model name with that state suffix
 * already cut; state_level[u] (HOST): the file's first line had a state suffix.  The rows of an utterance are its
 * lines' [start, end) ranges one after another -- lines are not checked against each other, as in the script -- so
 * the sum of end - start must equal the utterance's frame count.  A state-level line's phoneme reaches back while the
 * previous line's state index is smaller and forward while the next one's is larger (:300-316); in a phoneme-level
 * file every line is its own phoneme, whatever its state index (the script's misspelt level check lets such lines in).
 * out: DEVICE float32, row t of the batch at out + t * ld_out, columns [0, n_features) written and nothing else; 16-byte
 * stores where ld_out and the pointer allow, the same bits either way.  status: NULL, or DEVICE int[n_utt]: bit 1 a
 * value of the utterance was clamped to 0 or 1 (the "Out of range" warning), bit 2 a state-related reserved feature
 * (kinds 2 .. 5) met a phoneme-level file and took the value min (the "There is not state-level information" warning).
 * No result depends on the batch around an utterance or on how names repeat.  Distinct names are found inside the
 * call, on the host.  A NULL required pointer, a set of another context, ld_out < n_features, end <= start, start < 0,
 * lines that do not add up to the frame count, an empty name: WM_ERR_BAD_ARG; a name longer than 1023 bytes or with a
 * byte outside 0x21-0x7E: WM_ERR_UNSUPPORTED; all before any device call.  Asynchronous on the context's stream after
 * its uploads (a second call on the same batch first waits for the first one's work); a batch of zero frames returns
 * WM_OK.  Timed as "label_match_kernel" and "ffi_rows_kernel". */
int WorldMi355LabelFeatures(WorldMi355Batch* b, const WorldMi355LabelFeatureSet* set, const int* line_off,
                            const int* start, const int* end, const int* state_index, const char* const* name,
                            const int* state_level, float* out, int64_t ld_out, int* status);
/* One pattern against one name (host only: no context, no HIP call).  pattern and is_float as in a feature; engine 0 is
 * the backtracking matcher, engine 1 the bit-parallel program of label_match_kernel stepped on the host through the
 * kernel's own step function (binary patterns only: WM_ERR_BAD_ARG with is_float).  *matched: 0 / 1; *value (may be
 * NULL): what %d captured, 0 otherwise.  Refusals as above. */
int WorldMi355LabelPatternMatch(const char* pattern, int is_float, const char* name, int engine, int* matched,
                                int* value);

/* The 12-byte HTK header of addhtkheader.pl:60-75 (host only, native byte order). */
void WorldMi355HtkHeader(int n_frames, int sampling_rate, int frame_shift_samples, int bytes_per_frame,
                         int htk_type, unsigned char out12[12]);

/* The fwrite loops at the end of the reference's `analysis` CLI (test/analysis.cpp:360-390), for a whole batch at
 * once: file i = paths[i] receives bytes[i] bytes from data[i] (HOST memory: the pinned slabs a sweep copies the
 * float32 features into), created or truncated.  n_threads plain threads work the list off; returns when every
 * file is written and closed.  Host only: no context, no HIP call.  WM_ERR_IO names the first file that failed. */
int WorldMi355WriteFiles(int n_files, const char* const* paths, const void* const* data, const size_t* bytes,
                         int n_threads);


/* ---- Vibrato feature (data/scripts/Extract.py:115-227, invoked at data/Makefile.in:215), SURVEY.md 8(f) rank 4 ----
 * lf0: DEVICE, float32 [total_frames], log f0 with 0 for unvoiced frames (WorldMi355RecipeFeatures' lf0).
 * Label segments: HOST arrays.  Utterance u owns segments seg_utt_off[u] .. seg_utt_off[u+1]-1 (n_utt + 1 offsets);
 * segment s covers frames [seg_start[s], seg_end[s]) of its utterance (floor(label time / frame period), clamped as
 * Extract.py:181-182) and has note pitch seg_pitch[s] in Hz (0 for "xx").
 * Outputs (DEVICE, float32, after the script's soprLog): vib [total_frames][2] = log depth, log period;
 * lf0_out [total_frames][2] = log f0, log(f0 - pitch + 500) -- what the script writes back over the lf0 file.
 * *n_too_long (may be NULL): voiced runs longer than 3072 frames, left without vibrato.  Synchronises the stream.
 * Parity of this entry point is UNPINNED: the reference holds no fixtures for it and its LOWESS is an unpinned
 * third-party dependency (statsmodels); DESIGN.md section 4. */
int WorldMi355Vibrato(WorldMi355Batch* b, const float* lf0, const int* seg_utt_off, const int* seg_start,
                      const int* seg_end, const double* seg_pitch, float* vib, float* lf0_out, int* n_too_long);

/* Per-kernel timing with HIP events recorded on the context's stream around each launch of the
 * named kernels ("dio_lowcut_kernel", "dio_band_kernel", "stonemask_kernel", "cheaptrick_kernel",
 * "d4c_lovetrain_kernel", "d4c_kernel", "synth_timebase_kernel", "synth_pulse_kernel",
 * "synth_ola_kernel", "mcep_kernel", "mgcep_kernel", "mlpg_kernel", "mcpf_kernel", "modify_kernel", "mspf_kernel", "mspf_stats_kernel",
 * "interpolate_gaps_kernel", "ffo_compose_kernel", "column_moments_kernel", "trj_kernel": its
 * column kernels and trj_reduce_kernel as one record, "dnn_layer_kernel": all layers of a call as one record,
 * "dnn_cost_kernel", "optimizer_step_kernel", "label_match_kernel", "ffi_rows_kernel").  Enable clears earlier records; Query synchronises the stream and
 * returns the summed duration and the number of launches since Enable. */
int WorldMi355TimingEnable(WorldMi355Context* ctx, int on);
int WorldMi355TimingQuery(WorldMi355Context* ctx, const char* kernel, double* total_ms, int* launches);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WORLD_MI355_H_ */
