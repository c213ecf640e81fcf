/* libkws_hip.so - C ABI of the MI355X (gfx950) keyword-spotting hot path.
 *
 * The reference (see--/speech_recognition) has no FFI of its own: its hot path is Python that
 * lowers to TensorFlow-1.4 / Keras-2.1.2 ops.  Each entry point below replaces the
 * ops behind one reference call site, cited as file:line under the reference checkout.
 *
 * Conventions
 *  - plain C, no exceptions across the ABI; every function returns 0 (KWS_OK) or a negative
 *    KWS_E_* code; kws_last_error() returns a thread-local message for the last failure.
 *  - every tensor argument is a raw DEVICE pointer owned by the caller (e.g. the data_ptr() of a
 *    PyTorch-ROCm tensor); the library never frees or retains it.  Exceptions are the *_create
 *    functions, whose table arguments are HOST pointers copied once into a plan.
 *  - work is enqueued on `stream` (a hipStream_t passed as void*) and not synchronised.
 *  - layout is channels-last row-major fp32 [B, L, C] (= Keras channels_last), so Keras-named
 *    weights load without transposes: conv1d/kernel [k, Cin, Cout], depthwise_kernel [1,3,C,1],
 *    dense/kernel [in, out].
 *  - functions are re-entrant: no global mutable state besides the thread-local error string and the
 *    thread-local profiler attachment; switches (profiling, GEMM arithmetic arm) live on handles.
 */
#ifndef KWS_HIP_H_
#define KWS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libkws_hip.so is built with -fvisibility=hidden: exactly the declarations of this header are exported
 * (tests/test_abi.py compares `nm -D` with it) */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define KWS_OK 0
#define KWS_E_INVALID (-1)   /* bad argument / unsupported shape */
#define KWS_E_HIP (-2)       /* a HIP runtime call failed */
#define KWS_E_WORKSPACE (-3) /* caller workspace too small */

#define KWS_ABI_VERSION 5   /* round 6: round 5's measured loss (kws_wgrad_items_t, kws_dwconv_bwd_bn_wgrad_f32, kws_gemm_tn_items, kws_gemm_tn_ckpt_floats, gemm mode 3) retired from the ABI - kept as scripts/probes/wgrad_beside_dwbwd/mode3.patch; round 5 (4): a refused profiler_destroy changes nothing; round 4 (3): hidden visibility (exports = this header), the three |x|-maximum producers, gemm mode 1, profiler_destroy may refuse; round 3 (2): profiler / gemm-mode state moved onto handles */

int kws_abi_version(void);
const char* kws_last_error(void);
/* name of the device the calling thread is bound to; "" if no HIP device is usable */
int kws_device_name(char* buf, int cap);

/* A HIP stream in a scheduling class (cls: -1 lowest, 0 normal, +1 highest priority of the device's range).  The
 * batch generator runs on a LOW-priority stream so that its kernels fill the CUs the training stream leaves idle
 * instead of co-running with its MFMA kernels (PyTorch itself can only create normal / high priority streams). */
int kws_stream_create(int cls, void** stream);
int kws_stream_destroy(void* stream);

/* Optional per-kernel-family profiler (measurement only).  A profiler is a HANDLE; kws_profiler_attach(p) makes the
 * CALLING THREAD record into p (NULL detaches): while attached, every launcher called from that thread brackets its
 * launch with a hipEvent pair on the launch stream and books the algorithmic FLOPs/bytes of the call.  Several threads
 * may attach the same handle (the batch generator thread and the training thread of bench.py do).
 * kws_profiler_collect() waits for the recorded events and returns the number of families, kws_profiler_get() reads one
 * (summed device ms, launches, FLOPs, bytes).  No process-wide switch: a thread that never attaches never records.
 * The handle counts its attached threads (a thread that exits detaches itself): kws_profiler_destroy() returns KWS_E_INVALID
 * and changes NOTHING - the handle stays alive, the calling thread stays attached - while any OTHER thread is still attached;
 * when it succeeds it ends the calling thread's own attachment with the handle. */
typedef struct kws_profiler kws_profiler_t;
int kws_profiler_create(kws_profiler_t** out);
int kws_profiler_destroy(kws_profiler_t* p);
int kws_profiler_attach(kws_profiler_t* p);
int kws_profiler_collect(kws_profiler_t* p);
int kws_profiler_get(kws_profiler_t* p, int idx, char* name, int cap, double* ms, int64_t* count, double* flops,
                     double* bytes);

/* ------------------------------------------------------------------------------------------
 * a2  augment graph: decode_wav -> multiply -> tf_roll -> multiply/add -> reshape
 *     reference input_data.py:334-359, utils.py:56-73
 *   out[b,t] = bg_vol[b] * noise[noise_off[b] + t] + fg_vol[b] * bank[clip_idx[b], (t - shift[b]) mod L]
 * bank: [n_clips, L] resident clip bank (f32, or int16 PCM scaled by 1/32768 like DecodeWav).
 * noise: 1-D concatenation of the background recordings (input_data.py:274-309); noise_off are
 * absolute start samples (input_data.py:484-487); noise may be NULL when every bg_vol is 0.
 * A noise sample whose index noise_off[b] + t lies outside [0, noise_len) reads as 0 (a slice that starts before the
 * recording, runs off its end or misses it entirely is defined, and nothing outside noise[0, noise_len) is read).
 * shift may be any int32 (taken mod L).  out [B, L] must be 16-byte aligned when L % 4 == 0 (its rows are then written
 * with 16-byte stores; KWS_E_INVALID before any launch otherwise); any float alignment serves for other L.
 * ---------------------------------------------------------------------------------------- */
int kws_augment_f32(const float* bank, int64_t n_clips, int L, const int32_t* clip_idx,
                    const float* fg_vol, const int32_t* shift, const float* noise,
                    int64_t noise_len, const int64_t* noise_off, const float* bg_vol,
                    float* out, int B, void* stream);
int kws_augment_i16(const int16_t* bank, int64_t n_clips, int L, const int32_t* clip_idx,
                    const float* fg_vol, const int32_t* shift, const float* noise,
                    int64_t noise_len, const int64_t* noise_off, const float* bg_vol,
                    float* out, int B, void* stream);

/* a1  host-side sampler: the per-clip RNG draw loop of AudioProcessor.get_data, reference
 * input_data.py:457-514 (draw order: SURVEY Appendix C).  Pure host code (no GPU work): consumes the
 * NumPy legacy MT19937 stream passed in (key[624], pos as in np.random.get_state()) and advances it,
 * so seeded runs reproduce the reference's choices.  Outputs are the per-clip parameters of
 * kws_augment_* plus the label indices. */
typedef struct {
  const int32_t* rows;    /* clip-bank row of every entry of the partition */
  const int32_t* labels;  /* label index (word_to_index) */
  const uint8_t* silence; /* 1 where the entry is a _silence_ clip */
  int32_t n;
} kws_sampler_set_t;
typedef struct {
  int32_t deterministic;  /* 1: entries offset..offset+count-1 in order (how_many == -1 or mode != training) */
  int32_t offset, count;
  int32_t use_background; /* background data present and mode == training */
  int32_t n_bg;
  const int64_t* bg_len;   /* samples per background recording */
  const int64_t* bg_start; /* start of each recording inside the concatenated noise vector */
  int32_t desired_samples;
  int32_t shift_lo, shift_hi; /* time_shift_range (inclusive) */
  double background_frequency, background_volume_range, foreground_frequency, foreground_volume_range;
  double time_shift_frequency, pseudo_frequency, flip_frequency, silence_volume_range;
} kws_sampler_args_t;
int kws_sampler_draw(uint32_t* mt_key, int* mt_pos, const kws_sampler_set_t* cand,
                     const kws_sampler_set_t* pseudo, const kws_sampler_args_t* args,
                     int32_t* out_rows, int32_t* out_labels, int32_t* out_shift, int64_t* out_bg_off,
                     float* out_bg_vol, float* out_fg_vol);

/* a17 TTA transforms, reference make_submission.py:125-134.
 * kind: 0 copy, 1 np.roll(X,-1500,axis=1), 2 1.2*X, 3 clip(1.1*X,-1,1), 4 0.9*X */
int kws_tta_transform(const float* x, float* out, int B, int L, int kind, void* stream);
/* mean of n_terms probability tensors / divisor, argmax; make_submission.py:137-146.
 * out_probs[b,c] = (((probs[0] + probs[1]) + probs[2]) + ...)[b,c] / divisor in float32, in that order (the bits of an f32
 * NumPy evaluation); out_argmax[b] (may be NULL) is the FIRST index of the row's largest value, as np.argmax returns it.
 * 1 <= n_terms <= 8, divisor != 0. */
int kws_tta_combine(const float* const* probs, int n_terms, float divisor, float* out_probs,
                    int32_t* out_argmax, int B, int C, void* stream);

/* Speed-TTA time stretch: reference create_tta_set.py:9-22 -
 * librosa.effects.time_stretch(np.float32(pcm) / 32767, rate)[-keep:] -> np.int16(. * 32767) -> wav, read back
 * by make_submission.py:86-100 through DecodeWav (/ 32768) for the slow predict passes (:133-136).
 * librosa 0.5.x defaults (STFT 2048 / 512, periodic Hann, centred reflect padding, phase vocoder, ISTFT with
 * window-sum-square normalisation trimmed by 1024 each side); the stretched signal has
 * kws_stretch_out_samples() = 512 * (ceil((1 + n_samples / 512) / rate) - 1) samples.
 *   x   [B, n_samples] f32 (multiplied by in_scale on load) or int16 (divided by 32767 like the reference)
 *   out [B, keep]: the LAST `keep` stretched samples; zero padded at the end when fewer exist
 *   quantize != 0 reproduces the int16 wav round trip: (int16)(v * 32767) / 32768 (C-cast truncation)
 * rate <= 0 is KWS_E_INVALID (librosa raises ParameterError). */
typedef struct kws_stretch_plan kws_stretch_plan_t;
int kws_stretch_plan_create(int n_samples, double rate, kws_stretch_plan_t** plan);
int kws_stretch_plan_destroy(kws_stretch_plan_t* plan);
int kws_stretch_out_samples(const kws_stretch_plan_t* plan);
int kws_time_stretch_f32(const kws_stretch_plan_t* plan, const float* x, float in_scale, float* out, int B,
                         int keep, int quantize, void* stream);
int kws_time_stretch_i16(const kws_stretch_plan_t* plan, const int16_t* x, float* out, int B, int keep,
                         int quantize, void* stream);

/* Rational polyphase resampling of wav rows (csrc/resample.hip): scipy.signal.resample_poly(x, up, down) at its defaults
 * (window ('kaiser', 5.0), padtype 'constant').  g = gcd(rate_out, rate_in), up = rate_out / g, down = rate_in / g,
 * mx = max(up, down), half = 10 mx; the prototype has 2 half + 1 taps h[j] = up w[j] fc sinc(fc (j - half)) / S with
 * fc = 1 / mx, w = kaiser(2 half + 1, 5.0) and S the sum of the unscaled windowed taps;
 *   y[n] = sum_j h[j] xu[n down + half - j],  xu[i up] = x[i], zero elsewhere;  n_out = ceil(n_in up / down);
 * taps_per_phase = ceil((2 half + 1) / up) taps meet a sample per output.  Equal rates (up = down = 1) are a copy.
 * Rates < 1 or max(up, down) > 65536 are KWS_E_INVALID.
 * The first three calls are host-only (no device is touched).  The design and out_samples calls write / return the numbers
 * above (NULL pointers are skipped); the taps call returns the prototype in natural order, designed in double and rounded to
 * float once - the floats the kernels multiply with; n must be 2 half + 1. */
int kws_resample_design(int rate_in, int rate_out, int* up, int* down, int* half_len, int* taps_per_phase);
int kws_resample_taps(int rate_in, int rate_out, float* h, int64_t n);
int64_t kws_resample_out_samples(int rate_in, int rate_out, int64_t n_in);
/* The plan holds the phase-major device table of one rate pair (create it on the device that runs the launches).
 *   x        [B] rows x_pitch (>= n_in) elements apart; row b is read at [0, n_valid[b]) only
 *   n_valid  device [B] (clamped to [0, n_in]), or NULL = n_in for every row
 *   out      [B, keep]: the first `keep` resampled samples, zeros from ceil(n_valid up / down) on (a zero row for n_valid = 0)
 * int16 samples enter as integers (no 1 / 32768 scale).  out_i16 = clamp(rintf(v), -32768, 32767) (round half to even) of the
 * very v stored to out_f32; either may be NULL, not both.  Inputs must be finite.  No atomics, every element written once;
 * a row's bits do not depend on the batch around it. */
typedef struct kws_resample_plan kws_resample_plan_t;
int kws_resample_plan_create(int rate_in, int rate_out, kws_resample_plan_t** plan);
int kws_resample_plan_destroy(kws_resample_plan_t* plan);
int kws_resample_i16(const kws_resample_plan_t* plan, const int16_t* x, int64_t x_pitch, const int32_t* n_valid, int n_in,
                     int16_t* out_i16, float* out_f32, int B, int keep, void* stream);
int kws_resample_f32(const kws_resample_plan_t* plan, const float* x, int64_t x_pitch, const int32_t* n_valid, int n_in,
                     float* out, int B, int keep, void* stream);

/* Keyword spotting in a recording of any length (csrc/stream.hip; not in the reference, which infers one-second clips only).
 * The window gather: W overlapping windows of `win` samples, `hop` samples apart, the first one starting at sample `start`,
 *   out[w * win + i] = scale * (float)src[s],  s = start + (int64)w * hop + i,  an exact 0.0f where s is outside [0, n)
 * (one float multiply: the bits are defined).  start may be negative, hop may exceed win, n may be 0 or smaller than win; all
 * index arithmetic is 64-bit.  Nothing outside src[0, n) is read, nothing outside out[0, W * win) is written.
 * KWS_E_INVALID unless win % 4 == 0, win >= 4, hop >= 1, W >= 1, out is 16-byte aligned, src aligned to its element size and
 * 0 <= n <= 2^61, |start| <= 2^61 (the index above then fits int64 for every w).
 * scale: 1 / 32768 gives DecodeWav's floats from int16 samples. */
int kws_stream_frames_i16(const int16_t* src, int64_t n, int64_t start, int hop, int win, float scale, float* out, int W,
                          void* stream);
int kws_stream_frames_f32(const float* src, int64_t n, int64_t start, int hop, int win, float scale, float* out, int W,
                          void* stream);
/* The same gather as a copy of bits into rows `out_pitch` floats apart (the windows of a feature track that overlapping
 * windows share; two calls with one out_pitch assemble composite rows):
 *   out[w * out_pitch + i] = src[start + w * hop + i]  for 0 <= w < W, 0 <= i < win,  an exact +0.0f where that index is
 * outside [0, n).  No arithmetic: NaN payloads, -0.0 and denormals arrive unchanged.  Nothing outside src[0, n) is read;
 * nothing outside the W segments [w * out_pitch, w * out_pitch + win) is written - the out_pitch - win floats between the
 * rows stay the caller's.  Any win >= 1, hop >= 1, out_pitch >= win, W >= 1, 0 <= n <= 2^61, |start| <= 2^61; src and out
 * need float alignment only (16-byte stores are used wherever a row's own alignment allows).  KWS_E_INVALID otherwise, and
 * for an output of more than 2^61 floats ((W - 1) * out_pitch + win), which has no address.  All index arithmetic is 64-bit. */
int kws_stream_gather_f32(const float* src, int64_t n, int64_t start, int64_t hop, int win, float* out, int64_t out_pitch,
                          int W, void* stream);
/* Posterior smoothing and top-1 over a whole track probs [W, NC]:  lo = max(0, w - A + 1),
 *   smoothed[w, c] = (probs[lo, c] + ... + probs[w, c]) / (float)(w - lo + 1)
 * summed in ascending row order in float32, one correctly rounded float32 division; top[w] = the lowest c that attains the
 * maximum of smoothed[w, :], top_score[w] = that maximum.  smoothed may be NULL.  1 <= A <= 4096, 1 <= NC <= 256, W >= 1.
 * Every output is the direct A-term sum (no carried running sum), no atomics: a row's bits depend only on the rows under it. */
int kws_stream_smooth_f32(const float* probs, int W, int NC, int A, float* smoothed, int* top, float* top_score, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone forms of the classifier-tail ops (the network programs below run them fused in one
 * kernel; these bind ONE reference call site each).
 *
 * keras Dropout, reference model.py:819,828 (mask = floor(keep_prob + U[0,1)), x / keep_prob).
 * Counter-based: element i of row r keeps its value iff fmix32(((row_offset + r) * n + i) * 0x9E3779B1 + key) <
 * keep_prob * 2^32, key = f(seed, step, layer_id) - the masks the network programs and the oracle use
 * (layer_id 1 = dropout_1, 2 = dropout_2).  bwd = the same mask applied to the incoming gradient.
 * ---------------------------------------------------------------------------------------- */
int kws_dropout_fwd(const float* x, float* out, int B, int n, float keep_prob, uint64_t seed,
                    uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream);
int kws_dropout_bwd(const float* dy, float* dx, int B, int n, float keep_prob, uint64_t seed,
                    uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream);

/* a12 attention pooling, reference model.py:824-827:
 *   feat[b] = [ max_t(x[b,t,:] * att[b,t]) ; mean_t x[b,t,:] ]        x [B,T,C], att [B,T], feat [B,2C]
 * bwd: dfeat [B,2C] -> dx [B,T,C] (gradient wrt x through both branches) and datt [B,T]; reduce_max
 * splits its gradient equally among ties (TF _MinOrMaxGrad).  workspace: kws_attn_pool_bwd_workspace_floats. */
int kws_attn_pool_fwd(const float* x, const float* att, float* feat, int B, int T, int C, void* stream);
int64_t kws_attn_pool_bwd_workspace_floats(int B, int T, int C);
int kws_attn_pool_bwd(const float* x, const float* att, const float* dfeat, float* dx, float* datt,
                      float* workspace, int B, int T, int C, void* stream);

/* a13 smooth_categorical_crossentropy, reference utils.py:87-108 as used at model.py:835-836:
 *   loss[b] = softmax_cross_entropy(labels = y (1 - s) + s / NC, logits = log(clip(p, 1e-7, 1 - 1e-7)))
 * probs/labels [B,NC] (NC <= 64); per_correct (may be NULL) = 1 where argmax p == argmax y.
 * bwd: dprobs = dL/dp * inv_loss_batch (zero where the clip is active), dlogits = that gradient carried
 * through the softmax that produced p; either output may be NULL. */
int kws_softmax_xent_smooth_fwd(const float* probs, const float* labels, float* per_loss,
                                float* per_correct, int B, int NC, float label_smoothing, void* stream);
int kws_softmax_xent_smooth_bwd(const float* probs, const float* labels, float* dprobs, float* dlogits,
                                int B, int NC, float label_smoothing, float inv_loss_batch, void* stream);

/* Gradient exchange of the data-parallel step (the reference is single-session, train.py:24-26):
 * an RCCL communicator from a (rank, world, 128-byte unique id) triple - rank 0 calls kws_comm_unique_id and
 * hands the bytes to the other ranks by any side channel - and the in-place sum of the flat gradient buffer
 * over xGMI, enqueued on `stream`.  librccl is resolved at run time (dlopen); a process that never creates a
 * communicator never loads it. */
typedef struct kws_comm kws_comm_t;
int kws_comm_unique_id(void* id128);
int kws_comm_create(int rank, int world, const void* id128, kws_comm_t** comm);
int kws_comm_destroy(kws_comm_t* comm);
int kws_allreduce_grads(kws_comm_t* comm, float* grads, int64_t n, void* stream);

/* a18 32->12 head, reference freeze_graph_32_classes.py:55-69.
 * map[i] in [0,12): output slot of input class i (slot 1 = max over all classes mapped to 1). */
int kws_head32to12(const float* p_in, int C_in, const int32_t* map, int C_out, float* p_out,
                   int B, void* stream);

/* ------------------------------------------------------------------------------------------
 * a3-a5  STFT -> |X| -> mel -> log -> DCT   (one table-driven kernel for both feature paths)
 *     path B: reference input_data.py:361-381 (tf.contrib.signal.stft, abs, tensordot mel,
 *             log(+1e-6), mfccs_from_log_mel_spectrograms[..., :K])
 *     path A: reference audio.py:15-23 (audio_spectrogram magnitude_squared -> mfcc)
 * Host tables (copied into the plan): window[frame_len], mel[n_bins * n_mel] row-major
 * (n_bins = fft_len/2+1), dct[n_mel * n_out] row-major.  fft_len must be 512.
 * out_kind: 0 = DCT features [B,F,n_out] (mfcc_), 1 = magnitude spectrogram [B,F,257]
 * (spectrogram_, input_data.py:366), 2 = log-mel [B,F,n_mel].
 * ---------------------------------------------------------------------------------------- */
typedef struct kws_stft_plan kws_stft_plan_t;
int kws_stft_plan_create(int frame_len, int frame_step, int fft_len, int n_mel, int n_out,
                         const float* window, const float* mel, const float* dct,
                         float log_offset, float log_floor, kws_stft_plan_t** plan);
int kws_stft_plan_destroy(kws_stft_plan_t* plan);
int kws_stft_num_frames(const kws_stft_plan_t* plan, int L);
int kws_stft_mel_f32(const kws_stft_plan_t* plan, const float* x, int B, int L, float* out,
                     int out_kind, void* stream);
/* Which kernel kws_stft_mel_f32 launches for (plan, x, L, out_kind); host arithmetic only, nothing
 * is launched and kws_stft_mel_f32 itself decides through this function.  Not an error code:
 *   0 / 1                  the generic kernel with 4 / 7 waves per workgroup (7: F % 14 == 0)
 *   10 + 2 * shape + v4    the register-FFT kernel: shape 1..4 = its mel-band instance
 *                          (80-band form, 5 lane groups at full width, 40-band form, 3 lane groups at
 *                          full width), v4 = 1 with 16-byte PCM loads (L % 4 == 0, frame_step % 4 == 0,
 *                          x 16-byte aligned), 0 with 8-byte loads
 *   -1                     arguments kws_stft_mel_f32 refuses */
int kws_stft_mel_kernel(const kws_stft_plan_t* plan, const float* x, int L, int out_kind);

/* A/B arm, off by default (csrc/gemm_f16x2.hip; selected per net handle by kws_net_set_gemm_mode(net, 2)): the pointwise
 * GEMMs with every f32 operand scaled by a power of two and split into TWO fp16 parts, three f16 MFMA products
 * accumulated in f32 - as accurate as the f32 matrix pipe, not bit-identical to it.  The scale of an operand
 * comes from its |x| maximum, kept on the device in a "slot group" of 256 words (atomicMax of the bit patterns, so it
 * is the same in every run): kws_absmax_batch_f32 fills groups for arbitrary tensors; inside the network the kernels
 * that produce a GEMM operand leave its maximum behind.  The largest magnitude lands in [2^14, 2^15) (fp16 overflows at
 * 65504) and results are multiplied by the two inverse scales on the way out (exact: powers of two). */
int kws_absmax_batch_f32(const float* const* in, const int64_t* n, unsigned* slots, int count, void* stream);
/* The producers of a GEMM operand that leave the operand's |x| maximum behind on the way (what the network programs call for this
 * arm; `amax` = a slot group of 256 words zeroed by the caller, or NULL = the plain kernel): kws_dwconv_fwd_f32 / pass 2 of
 * kws_dwconv_bwd_bn_f32 / kws_bn_bwd_apply with one more argument.  The tensors they write are bit-identical to the plain calls'. */
int kws_dwconv_fwd_amax_f32(const float* y, const float* bn, const float* w, float* z, int B, int L_in, int L_out,
                            int C, int stride, int pad_l, unsigned* amax, void* stream);
int kws_dwconv_bwd_bn_amax_f32(const float* dz, const float* y, const float* bn, const float* w, const float* coef,
                               float* dy, float* part, int pass, int B, int L_in, int L_out, int C, int stride, int pad_l,
                               unsigned* amax, void* stream);
int kws_bn_bwd_apply_amax(float* g, const float* y, const float* bn, const float* gamma, const float* coef, int64_t rows,
                          int C, unsigned* amax, void* stream);
int kws_f16x2_split_batch(const float* const* in, void* const* out, const int* rows, const int* cols,
                          const int* transpose, const unsigned* const* slots, int count, void* stream);
/* shapes the arm's kernels take (K granule, 32-bit offsets inside a 2 GB buffer view); the network programs fall back
 * to the f32 kernels for anything else.  stats rows of the NN kernel: one per 128-row tile. */
int kws_gemm_nn_f16x2_supported(int64_t M, int K, int N);
int kws_gemm_tn_f16x2_supported(int64_t M, int K, int N);
int kws_gemm_nn_f16x2_stats_rows(int64_t M);
int kws_gemm_nn_f16x2_f32(const float* A, const void* Bp, float* C, int64_t M, int K, int N,
                          const unsigned* a_slots, const unsigned* b_slots, float* stats_part, void* stream);
int64_t kws_gemm_tn_f16x2_workspace_floats(int64_t M, int K, int N);
int kws_gemm_tn_f16x2_f32(const float* Z, const float* G, float* dW, int64_t M, int K, int N,
                          const unsigned* z_slots, const unsigned* g_slots, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * a7+a8, a10  GEMM family on f32 MFMA (v_mfma_f32_32x32x2_f32)
 *   C[M,N] = A[M,K] * W[K,N]          pointwise Conv1D(1x1)  reference model.py:48-49
 *   with a gathered A it is frame+Conv1D(k3,s2) (model.py:805-808) / Conv1D(64,3) (model.py:1450)
 *   / the stride-2 1x1 shortcut (model.py:1431-1432):
 *   A[(b,t), j*cin + c] = X[b*x_batch_stride + t*stride_t + j*stride_j + c + base_off], 0 outside
 *   [0, x_len) of clip b.
 * stats (optional, may be NULL): partial column sums [rows][2][N] (sum x, sum x^2) for BatchNorm, finalised
 * by kws_bn_stats_finalize (a11).  The buffer must hold 2 * kws_gemm_num_row_tiles(M) * N floats (an upper
 * bound); the number of rows a call actually writes is kws_gemm_nn_stats_rows(M, K, N) for kws_gemm_nn_f32
 * (one row per workgroup of the persistent kernel, <= 256) and kws_gemm_gather_stats_rows(M) for
 * kws_gemm_gather_f32 (one row per 128-row tile) - pass that count to kws_bn_stats_finalize.
 * ---------------------------------------------------------------------------------------- */
int kws_gemm_num_row_tiles(int64_t M);
int kws_gemm_nn_stats_rows(int64_t M, int K, int N);
int kws_gemm_gather_stats_rows(int64_t M);
int kws_gemm_nn_f32(const float* A, const float* W, float* C, int64_t M, int K, int N,
                    float* stats_part, void* stream);
typedef struct {
  int L_out;             /* rows per clip */
  int cin;               /* channels per tap */
  int taps;              /* K = taps * cin */
  int stride_t;          /* element stride between consecutive output rows */
  int stride_j;          /* element stride between taps */
  int base_off;          /* offset of (t=0, j=0, c=0), may be negative (SAME padding) */
  int x_len;             /* valid elements per clip */
  int64_t x_batch_stride;
} kws_gather_t;
int kws_gemm_gather_f32(const float* X, const kws_gather_t* g, const float* W, float* C, int B,
                        int N, float* stats_part, void* stream);
/* dW[K,N] = A^T[K,M] * G[M,N] (Conv2DBackpropFilter of the 1x1 conv); deterministic split-M:
 * workspace floats >= kws_gemm_tn_workspace_floats(M,K,N). */
int64_t kws_gemm_tn_workspace_floats(int64_t M, int K, int N);
int kws_gemm_tn_f32(const float* A, const float* G, float* dW, int64_t M, int K, int N,
                    float* workspace, void* stream);
int kws_gemm_tn_gather_f32(const float* X, const kws_gather_t* g, const float* G, float* dW, int B,
                           int N, float* workspace, void* stream);
int kws_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped Conv1D (VALID, no bias) on f32 MFMA: the g Keras Conv1D layers of the reference's _grouped_reduce_conv /
 * _grouped_context_conv (model.py:651-693, 1258-1300), each reading the slice x[:, :, q*gs : (q+1)*gs] of one input and
 * concatenated in group order.  Input X [B, L, C]; output [B, Lout, F = g*Ng], group q at columns q*Ng.  Kernel of group q:
 * [k, gs, Ng] (Keras layout) at W + q * w_group_stride (0 = k*gs*Ng: the groups back to back).  Channels >= g*gs are never
 * read.  One launch covers all groups; results are bit-identical from run to run (no atomics).
 *   fwd    Y[b,t,q*Ng+n] = sum_{j,c} act(X[b, stride*t + j, q*gs + c]) * W_q[j,c,n]; act = relu6(scale*x + shift) of the
 *          producer's BatchNorm tables bn [C / bn_group][4][bn_group] (scale|shift|mean|rstd per BN layer of bn_group
 *          channels), or identity when bn is NULL.  stats_part (may be NULL): [kws_gconv_stats_rows][2][F] column sums
 *          (sum y, sum y^2) per 128-row tile for kws_bn_stats_finalize-style folding.
 *   dgrad  dX[b,tau,q*gs+c] = sum over s*t + j = tau of sum_n dY[b,t,q*Ng+n] * W_q[j,c,n]: the gradient wrt the INPUT of
 *          the convolution (wrt act(X) when the forward applied a table).  Every element of dX is written: rows no
 *          window covers and channels >= g*gs are exact zeros.
 *   wgrad  dW_q[j,c,n] = sum_{b,t} act(X[b, stride*t+j, q*gs+c]) * dY[b,t,q*Ng+n], written at dW + q * w_group_stride;
 *          workspace >= kws_gconv_wgrad_workspace_floats floats (fixed-order split over B*Lout).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int B, L, C;     /* input [B, L, C] */
  int Lout;        /* output rows per clip: stride*(Lout-1) + k <= L */
  int k, stride;   /* taps, time stride */
  int g, gs, Ng;   /* groups, input channels per group, filters per group */
  int64_t w_group_stride;
} kws_gconv_t;
int kws_gconv_stats_rows(const kws_gconv_t* d);
int kws_gconv_fwd_f32(const float* X, const float* bn, int bn_group, const float* W, float* Y, float* stats_part,
                      const kws_gconv_t* d, void* stream);
int kws_gconv_dgrad_f32(const float* dY, const float* W, float* dX, const kws_gconv_t* d, void* stream);
int64_t kws_gconv_wgrad_workspace_floats(const kws_gconv_t* d);
int kws_gconv_wgrad_f32(const float* X, const float* bn, int bn_group, const float* dY, float* dW, float* workspace,
                        const kws_gconv_t* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped depthwise Conv1D (VALID, no bias): the depthwise halves of the g _depthwise_conv_block calls inside the reference's
 * _grouped_reduce_conv / _grouped_context_conv of conv_1d_top_down_model (model.py:1335-1373).  Input X [B, L, C]; output
 * Z [B, Lout, g*gs], group q at columns q*gs, made for a grouped 1x1 convolution (kws_gconv_* with k = 1) behind it.  Kernel of
 * group q: [k, gs] at w + q * w_group_stride (0 = k*gs: back to back; larger: the groups' other tensors lie in between and are
 * never touched).  Group q reads the channel window [x0 + q*x_step, + gs) of X: x_step = gs is the sliced form (a reduce block),
 * x_step = 0 the shared form (a context block: the reference passes x, not the slice, to every group, so every group filters
 * the same window with its own kernel).  Channels outside every window are never read.
 *   act    what a value of X goes through on load: KWS_GDW_ACT_NONE identity; KWS_GDW_ACT_BN_RELU6 relu6(scale*x + shift) of
 *          the producer's tables tab [C / bn_group][4][bn_group] (the form kws_gconv_fwd_f32 takes; indexed per channel, so
 *          bn_group need not be a multiple of 4); KWS_GDW_ACT_BIAS x + tab[ch], tab [C] a convolution's bias, no gate.
 *   fwd    Z[b,t,q*gs+c] = sum_j w_q[j,c] * act(X[b, stride*t + j, x0 + q*x_step + c]).  Shared form: X is read once per output
 *          tile for all groups.
 *   bwd    dA[b,u,ch] = sum over the groups q whose window holds ch (ascending) and the taps j with stride | (u - j) of
 *          w_q[j,c] * dZ[b,(u-j)/stride,q*gs+c]: the gradient wrt act(X), no gate applied (kws_gconv_dgrad_f32's contract; the
 *          BatchNorm backward does the gate).  Every element of dA [B, L, C] is written exactly once: rows no window reaches
 *          and channels no group reads are exact zeros.
 *          dW_q[j,c] = sum_{b,t} act(X[b, stride*t+j, ...]) * dZ[b,t,q*gs+c], written at dW + q * w_group_stride through
 *          kws_gdwconv_bwd_part_rows partial rows [k + 1][g*gs] (row k: column sums of dZ) in workspace, added in one fixed
 *          order.  dbias (may be NULL; KWS_GDW_ACT_BIAS only) [C]: the column sums of dA, taken from the same partial rows.
 *          workspace >= kws_gdwconv_bwd_workspace_floats floats (0 = outside the domain).
 * Domain: 1 <= k <= 7, 1 <= stride <= 4, 1 <= g <= 8; gs, C, x0, x_step multiples of 4; x0 + (g-1)*x_step + gs <= C;
 * stride*(Lout-1) + k <= L; X, Z, dZ, dA, workspace 16-byte aligned.  Anything else is KWS_E_INVALID before any launch.
 * No atomics: results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
#define KWS_GDW_ACT_NONE 0
#define KWS_GDW_ACT_BN_RELU6 1
#define KWS_GDW_ACT_BIAS 2
typedef struct {
  int B, L, C;     /* input [B, L, C] */
  int Lout;        /* output rows per clip: stride*(Lout-1) + k <= L */
  int k, stride;   /* taps, time stride */
  int g, gs;       /* groups, channels per group */
  int x0, x_step;  /* group q reads the channels [x0 + q*x_step, + gs) */
  int act;         /* KWS_GDW_ACT_* */
  int bn_group;    /* KWS_GDW_ACT_BN_RELU6: channels per table of tab */
  int64_t w_group_stride;
} kws_gdwconv_t;
int     kws_gdwconv_fwd_f32(const float* X, const float* tab, const float* w, float* Z, const kws_gdwconv_t* d, void* stream);
int     kws_gdwconv_bwd_part_rows(const kws_gdwconv_t* d);
int64_t kws_gdwconv_bwd_workspace_floats(const kws_gdwconv_t* d);
int     kws_gdwconv_bwd_f32(const float* X, const float* tab, const float* dZ, const float* w, float* dA, float* dW, float* dbias,
                            float* workspace, const kws_gdwconv_t* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * MaxPool1D(pool_size=3, strides=2, padding='valid') over relu6(bn(y)): the pool of the reference's _reduce_conv in
 * conv_1d_time_stacked_model / conv_1d_heavy_model (model.py:271-277, 423-429).  y [B, L, C] is the RAW convolution output,
 * bn its table scale|shift|mean|rstd [4][C]; C % 4 == 0, C <= 1024, L >= 3.
 *   fwd  z[b,t,c] = max_{j<3} relu6(scale[c] * y[b, 2t+j, c] + shift[c]), t < kws_pool3s2_out_len(L) = (L - 3) / 2 + 1.  The
 *        activation is applied BEFORE the maximum (a scale may be negative).  With an even L the last row is in no window.
 *   bwd  g[b,u,c] = relu6'(bn(y[b,u,c])) * sum of dz[b,t,c] over the windows t that row u won; the FIRST maximum of a window wins
 *        (TF MaxPoolGrad).  Every element of g [B, L, C] is written once (rows no window covers: exact 0).  part receives
 *        kws_pool3s2_bwd_part_rows() rows [2][C] of (sum g, sum g * xhat), xhat = (y - mean) * rstd: the BatchNorm backward's
 *        reductions, to be added over the rows in a fixed order.  No atomics: results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int kws_pool3s2_out_len(int L);
int kws_pool3s2_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream);
int kws_pool3s2_bwd_part_rows(int B, int L, int C);
int64_t kws_pool3s2_bwd_part_floats(int B, int L, int C);
int kws_pool3s2_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * MaxPool1D(pool_size=3, strides=2, padding='same') over relu6(bn(y)): the pool of the reference's _reduce_conv in
 * conv_1d_multi_time_sliced_model (model.py:1093-1097).  The contract of kws_pool3s2_* with TensorFlow's SAME geometry:
 * kws_pool3s2_same_out_len(L) = ceil(L / 2) windows, pad_left = 0 for an even L and 1 for an odd L; window t covers the rows
 * 2t - pad_left + j, j < 3, that exist (padding never wins; the middle row always exists).  C % 4 == 0, C <= 1024, L >= 2.
 *   fwd  z[b,t,c] = max over the window's valid rows of relu6(scale[c] * y[b,r,c] + shift[c]): the activation BEFORE the maximum.
 *   bwd  g[b,u,c] = relu6'(bn(y[b,u,c])) * sum of dz[b,t,c] over the windows t that row u won; the FIRST maximum among a window's
 *        valid rows wins (TF MaxPoolGrad).  Every element of g [B, L, C] is written once.  part receives
 *        kws_pool3s2_same_bwd_part_rows() rows [2][C] of (sum g, sum g * xhat) for the BatchNorm backward, to be added in a fixed
 *        order.  No atomics: results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int kws_pool3s2_same_out_len(int L);
int kws_pool3s2_same_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream);
int kws_pool3s2_same_bwd_part_rows(int B, int L, int C);
int64_t kws_pool3s2_same_bwd_part_floats(int B, int L, int C);
int kws_pool3s2_same_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense Conv1D (stride 1, no bias) with zero padding, dilation and channel windows, on f32 MFMA: the convolutions of the
 * reference's _inception_block / _reduce_inception_block (model.py:312-406), whose branches read one joined tensor and write
 * the slices of the next.  X [B, L, Cx], of which the columns [x0, x0 + Cin) are read; Y and dY [B, Lout, Cy], of which the
 * columns [y0, y0 + F) are written / read.  Kernel W [k, Cin, F] (Keras layout).  Lout = L + pad_l + pad_r - dil*(k-1) for
 * some 0 <= pad_r <= dil*(k-1); 0 <= pad_l <= dil*(k-1) (TF SAME: pad_l = dil*(k-1) / 2, Lout = L; VALID: pad_l = 0,
 * Lout = L - dil*(k-1)).  k 1..7, dil 1..4, any positive Cin / F.  Results are bit-identical from run to run (no atomics).
 *   fwd    Y[b,t,y0+n] = sum_{j,c} act(X[b, t - pad_l + dil*j, x0+c]) * W[j,c,n]; a tap outside [0, L) contributes 0 (the
 *          padding is zeros of the ACTIVATED tensor).  act = relu6(scale*x + shift) of the table bn [4][Cx]
 *          (scale|shift|mean|rstd, indexed by x0+c), or the identity when bn is NULL.  No other column of Y is touched.
 *          stats_part (may be NULL): [kws_conv1d_stats_rows][2][F] column sums (sum y, sum y^2) per 128-row tile.
 *   dgrad  dX[b,tau,x0+c] = sum_j sum_n dY[b, tau + pad_l - dil*j, y0+n] * W[j,c,n]: the gradient wrt act(X) (no gate is
 *          applied).  accumulate 0 overwrites the window, 1 adds to what is there; every element of the window is touched
 *          exactly once by one thread, no other column of dX is touched.
 *   wgrad  dW[j,c,n] = sum_{b,t} act(X[b, t - pad_l + dil*j, x0+c]) * dY[b,t,y0+n];
 *          workspace >= kws_conv1d_wgrad_workspace_floats floats (fixed-order split over B*Lout).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int B, L, Lout;      /* clips, input rows, output rows per clip */
  int k, dil, pad_l;   /* taps, dilation, zero rows in front of a clip */
  int Cx, x0, Cin;     /* row pitch of X, first column read, columns read */
  int Cy, y0, F;       /* row pitch of Y / dY, first column written, filters */
} kws_conv1d_t;
int kws_conv1d_stats_rows(const kws_conv1d_t* d);
int kws_conv1d_fwd_f32(const float* X, const float* bn, const float* W, float* Y, float* stats_part, const kws_conv1d_t* d,
                       void* stream);
int kws_conv1d_dgrad_f32(const float* dY, const float* W, float* dX, int accumulate, const kws_conv1d_t* d, void* stream);
int64_t kws_conv1d_wgrad_workspace_floats(const kws_conv1d_t* d);
int kws_conv1d_wgrad_f32(const float* X, const float* bn, const float* dY, float* dW, float* workspace, const kws_conv1d_t* d,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * AveragePooling1D(pool_size=3, strides=1, padding='same') over act(x): the pool branch of the reference's _inception_block.
 * x, z, dz, dx [B, L, C]; C % 4 == 0, L >= 1.  TensorFlow divides by the number n_t of rows that exist in window t: 3 inside
 * a clip, 2 at its ends (1 when L = 1).
 *   fwd  z[b,t,c] = (1 / n_t) * sum over r in {t-1, t, t+1} within [0, L) of act(x[b,r,c]); act = relu6(scale*x + shift) of the
 *        table bn [4][C], or the identity when bn is NULL.
 *   bwd  dx[b,u,c] = sum over t in {u-1, u, u+1} within [0, L) of dz[b,t,c] / n_t: the gradient wrt act(x) (no gate is applied).
 *        accumulate 0 overwrites dx, 1 adds to what is there.  No atomics: results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int kws_avgpool3_same_fwd_f32(const float* x, const float* bn, float* z, int B, int L, int C, void* stream);
int kws_avgpool3_same_bwd_f32(const float* dz, float* dx, int accumulate, int B, int L, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense NHWC Conv2D (no bias) on f32 MFMA: the convolution of the reference's MFCC-image models conv_2d_mobile / conv_2d_fast
 * (model.py:547-639).  X [B, H, W, Cin]; Y and dY [B, Hout, Wout, F]; kernel Wt [kh, kw, Cin, F] (Keras layout).  kh 1..20,
 * kw 1..8; strides sh, sw 1 or 2; dilations dh, dw 1 or 2, and 2 only on an axis whose stride is 1 (as TensorFlow requires); any
 * positive Cin / F.  Per axis the geometry is TensorFlow's SAME - out = ceil(in / s), total = max((out - 1)*s + d*(k - 1) + 1 -
 * in, 0), pad in front (pad_t / pad_l) = total / 2, the rest behind - or VALID: pad 0, out = (in - d*(k - 1) - 1) / s + 1.  A
 * descriptor whose Hout / Wout / pads do not follow from its other fields is refused.  Results are bit-identical from run to run
 * (no atomics).
 *   fwd    Y[b,p,q,n] = sum_{i,j,c} act(X[b, p*sh - pad_t + dh*i, q*sw - pad_l + dw*j, c]) * Wt[i,j,c,n]; a tap outside the
 *          image contributes 0 (the padding is zeros of the ACTIVATED tensor).  act: the identity when bn is NULL, else of the
 *          producer's table bn [4][Cin] (scale|shift|mean|rstd) relu6(scale*x + shift) (d->act = KWS_ACT_RELU6) or
 *          relu(scale*x + shift) (KWS_ACT_RELU).  stats_part (may be NULL): [kws_conv2d_stats_rows][2][F] column sums (sum y,
 *          sum y^2) per 128-row tile of M = B*Hout*Wout, for kws_bn_stats_finalize.
 *   dgrad  dX[b,y,x,c] = sum over (i,j,p,q) with p*sh - pad_t + dh*i = y, q*sw - pad_l + dw*j = x of sum_n dY[b,p,q,n] *
 *          Wt[i,j,c,n]: the gradient wrt act(X) (no gate is applied).  Every element of dX is written exactly once by one
 *          thread; rows and columns no window reads (stride 2 with a 1 x 1 or a VALID 3 x 3 window) get exact zeros.
 *   wgrad  dWt[i,j,c,n] = sum_{b,p,q} act(X[b, p*sh - pad_t + dh*i, q*sw - pad_l + dw*j, c]) * dY[b,p,q,n];
 *          workspace >= kws_conv2d_wgrad_workspace_floats floats (fixed-order split over M, then a fixed-order sum).
 * ---------------------------------------------------------------------------------------- */
#define KWS_ACT_RELU6 0
#define KWS_ACT_RELU 1
typedef struct {
  int B, H, W, Hout, Wout;   /* clips, input rows / columns, output rows / columns */
  int kh, kw;                /* window */
  int sh, sw;                /* strides */
  int dh, dw;                /* dilations */
  int pad_t, pad_l;          /* zero rows above / zero columns left of the image */
  int Cin, F;                /* input channels, filters */
  int act;                   /* KWS_ACT_*: the activation applied on load when a table is given */
} kws_conv2d_t;
int kws_conv2d_stats_rows(const kws_conv2d_t* d);
int kws_conv2d_fwd_f32(const float* X, const float* bn, const float* Wt, float* Y, float* stats_part, const kws_conv2d_t* d,
                       void* stream);
int kws_conv2d_dgrad_f32(const float* dY, const float* Wt, float* dX, const kws_conv2d_t* d, void* stream);
int64_t kws_conv2d_wgrad_workspace_floats(const kws_conv2d_t* d);
int kws_conv2d_wgrad_f32(const float* X, const float* bn, const float* dY, float* dWt, float* workspace, const kws_conv2d_t* d,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * MaxPool2D(pool_size=(2, 2), strides=2, padding='valid') over act(bn(y)): the pool of the reference's conv_2d_fast_model
 * (model.py:597-639).  The contract of kws_pool3s2_* in two dimensions.  y [B, H, W, C] is the RAW convolution output, bn its
 * table scale|shift|mean|rstd [4][C]; z and dz [B, H / 2, W / 2, C]; C % 4 == 0, C <= 1024, H >= 2, W >= 2; act is KWS_ACT_RELU6
 * or KWS_ACT_RELU.
 *   fwd  z[b,p,q,c] = max_{i,j<2} act(scale[c] * y[b, 2p+i, 2q+j, c] + shift[c]): the activation BEFORE the maximum (a scale may
 *        be negative).
 *   bwd  g[b,r,s,c] = act'(bn(y[b,r,s,c])) * dz[b, r/2, s/2, c] if (r, s) won its window, else 0; the FIRST maximum in row-major
 *        window order wins (TF MaxPoolGrad).  Every element of g [B, H, W, C] is written once; a last row or column that is in
 *        no window (odd H or W) gets exact 0.  part receives kws_pool2x2_bwd_part_rows() rows [2][C] of (sum g, sum g * xhat),
 *        xhat = (y - mean) * rstd: the BatchNorm backward's reductions, to be added over the rows in a fixed order.  No atomics:
 *        results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int kws_pool2x2_fwd_f32(const float* y, const float* bn, float* z, int B, int H, int W, int C, int act, void* stream);
int kws_pool2x2_bwd_part_rows(int B, int H, int W, int C);
int64_t kws_pool2x2_bwd_part_floats(int B, int H, int W, int C);
int kws_pool2x2_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int H, int W, int C, int act,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Framed first convolution at narrow widths: overlapping_time_slice_stack(x, ksize, hop, 'SAME') followed by
 * Conv1D(N, taps, strides=stride, 'valid', use_bias=False), the front end of the reference's conv_1d_time_sliced_model
 * (model.py:716-772: ksize 40, hop 20, taps 3, stride 2, N = 32 * filter_mult).  The frames are never materialised.
 *   fwd    y[b,t,n]  = sum_{j<taps} sum_{c<ksize} W[j,c,n] * x[b, hop*(stride*t + j) + c - pad_l]      (0 outside [0, L))
 *          stats_part (may be NULL): kws_frame_conv_stats_rows() rows [2][N] of (sum y, sum y^2) for kws_bn_stats_finalize
 *   wgrad  dW[j,c,n] = sum_{b,t} x[b, hop*(stride*t + j) + c - pad_l] * G[b,t,n]; overlapping taps each get their own
 *          gradient.  workspace >= kws_frame_conv_wgrad_workspace_floats() floats (fixed-order split over the row tiles,
 *          then a fixed-order sum): no atomics, bit-identical from run to run.  There is no input gradient (x is the waveform).
 * x: B clips of L samples, x_batch_stride apart (8-byte aligned); W and dW [taps, ksize, N] (Keras layout, unfolded); y and G
 * [B, Lout, N].  Domain: N 32 or 64; ksize, hop, taps >= 1 with span = hop*(taps-1) + ksize <= 128; stride 1 or 2; hop, pad_l
 * (>= 0) and x_batch_stride (>= L) even; hop*(stride*(Lout-1) + taps-1) + ksize - pad_l <= L + span.  Anything else returns
 * KWS_E_INVALID with nothing written (the planners return 0).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int B, L, Lout;          /* clips, samples per clip, output rows per clip */
  int ksize, hop, pad_l;   /* samples per frame, samples between frames, zeros in front of a clip */
  int taps, stride;        /* the Conv1D over the frames */
  int N;                   /* filters */
  int64_t x_batch_stride;
} kws_frame_conv_t;
int kws_frame_conv_stats_rows(const kws_frame_conv_t* d);
int kws_frame_conv_fwd_f32(const float* x, const float* W, float* y, float* stats_part, const kws_frame_conv_t* d, void* stream);
int64_t kws_frame_conv_wgrad_workspace_floats(const kws_frame_conv_t* d);
int kws_frame_conv_wgrad_f32(const float* x, const float* G, float* dW, float* workspace, const kws_frame_conv_t* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Banked strided first convolution: nbanks Conv1D(N, ksize[q], strides=stride, use_bias=False) layers over the raw waveform
 * whose outputs are concatenated, the filterbank front end of the reference's conv_1d_learned_spec_model (model.py:1159-1246:
 * six 'same' layers of 40 filters, 479 ... 161 taps, stride 160).  The banks are one banded product over one staged segment of
 * samples: a clip is read once, the structural zeros of a dense fold are not multiplied, y is written straight into the joined
 * tensor.
 *   fwd    y[b, t, q*N + n] = sum_{c < ksize[q]} W_q[c, n] * x[b, stride*t + c - pad_l[q]]      (0 outside [0, L))
 *   wgrad  dW_q[c, n]       = sum_{b, t} x[b, stride*t + c - pad_l[q]] * G[b, t, q*N + n]
 *          workspace >= kws_fbank_conv_wgrad_workspace_floats() floats (16-byte aligned; fixed-order split over the row tiles,
 *          then a fixed-order sum): no atomics, bit-identical from run to run.  Every element of every bank's dW_q is written,
 *          nothing between or around the banks is touched.  There is no input gradient (x is the waveform) and no statistics
 *          epilogue (no BatchNorm follows).
 * x: B clips of L samples, x_batch_stride apart (8-byte aligned; the floats between L and x_batch_stride are never read); bank
 * q's kernel W_q and gradient dW_q [ksize[q], 1, N] (Keras layout) at W + w_off[q] / dW + w_off[q]; y and G [B, Lout, nbanks*N].
 * TF SAME: Lout = ceil(L / stride), pad_l[q] = max((Lout - 1)*stride + ksize[q] - L, 0) / 2; VALID: pad_l 0.
 * Domain: 1 <= nbanks <= 8; N a multiple of 4, 4 <= N <= 64; stride even, 2 <= stride <= 4096; 1 <= ksize[q] <= 512,
 * 0 <= pad_l[q] < ksize[q] (either parity), w_off[q] >= 0; span = max(ksize - pad_l) + max(pad_l) <= 512; x_batch_stride even and
 * >= L; stride*(Lout - 1) < L + max(pad_l) (the last row's window starts inside the padded clip); B*Lout < 2^31.  Anything else
 * returns KWS_E_INVALID before any launch, with nothing written and no pointer dereferenced (the planner returns 0).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int B, L, Lout;            /* clips, samples per clip, output rows per clip */
  int stride;                /* samples between consecutive rows */
  int nbanks, N;             /* 1..8 banks of N filters each; output pitch F = nbanks * N */
  int ksize[8], pad_l[8];    /* per bank: taps, zeros in front of a clip (0 <= pad_l < ksize) */
  int64_t w_off[8];          /* per bank: offset in floats of its kernel [ksize, 1, N] (Keras layout) from W / dW */
  int64_t x_batch_stride;
} kws_fbank_conv_t;
int     kws_fbank_conv_fwd_f32(const float* x, const float* W, float* y, const kws_fbank_conv_t* d, void* stream);
int64_t kws_fbank_conv_wgrad_workspace_floats(const kws_fbank_conv_t* d);
int     kws_fbank_conv_wgrad_f32(const float* x, const float* G, float* dW, float* workspace, const kws_fbank_conv_t* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * GlobalAveragePooling1D over relu6(bn(y)) followed by Dropout: the head of the reference's conv_1d_time_sliced_model
 * (model.py:716-772), whose pooled features feed a hidden Dense layer.  y [B, T, C] is the RAW convolution output, bn its
 * table scale|shift|mean|rstd [4][C]; 1 <= T <= 16, C % 4 == 0, C <= 1024.
 *   fwd  feat[b,c] = (1/T) * sum_t relu6(scale[c] * y[b,t,c] + shift[c]);  fd[b,c] = feat[b,c] * mask(b,c) / keep_prob
 *   bwd  g[b,t,c]  = relu6'(bn(y[b,t,c])) * dfd[b,c] * mask(b,c) / (keep_prob * T), relu6' = [0 < pre <= 6].  Every element of g
 *        [B, T, C] is written once.  part receives kws_gap_drop_bwd_part_rows() rows [2][C] of (sum g, sum g * xhat), xhat =
 *        (y - mean) * rstd: the BatchNorm backward's reductions, to be added over the rows in a fixed order.
 * mask: kws_dropout_fwd's counter RNG on element (row_offset + b) * C + c, key from (seed, step, layer_id); keep_prob = 1: no
 * mask (inference).  No atomics: results are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int kws_gap_drop_fwd_f32(const float* y, const float* bn, float* feat, float* fd, int B, int T, int C, float keep_prob, uint64_t seed,
                         uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream);
int kws_gap_drop_bwd_part_rows(int B, int T, int C);
int kws_gap_drop_bwd_f32(const float* dfd, const float* y, const float* bn, float* g, float* part, int B, int T, int C, float keep_prob,
                         uint64_t seed, uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * a11  BatchNormalization (training: biased batch moments over (B,L); eps 1e-3; momentum .99)
 *      + Activation(relu6), reference model.py:46-51, 809-810; constants SURVEY D.2.
 * The normalise+ReLU6 is never materialised: it is applied on load by the consumer through the
 * per-channel (scale, shift) these functions produce.
 * bn layout: float[4*C] = scale | shift | mean | rstd.
 * ---------------------------------------------------------------------------------------- */
/* scratch (optional): KWS_REDUCE_SLICES * 2 * C floats (5 * C for kws_dw_bwd_finalize); when given,
 * long partial lists are folded in two fixed-order stages instead of one serial pass. */
#define KWS_REDUCE_SLICES 32
int kws_bn_stats_finalize(const float* stats_part, int n_tiles, int64_t count, int C,
                          const float* gamma, const float* beta, float eps, float momentum,
                          float* moving_mean, float* moving_var, float* bn, float* scratch,
                          void* stream);
int kws_bn_infer_prepare(const float* gamma, const float* beta, const float* moving_mean,
                         const float* moving_var, float eps, int C, float* bn, void* stream);
/* elementwise y -> relu6(scale*y+shift): only used by tests and by inference outputs */
int kws_bn_relu6_apply(const float* y, const float* bn, float* out, int64_t rows, int C, int relu6,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * a9  DepthwiseConv2D((1,3)) on [B,1,L,C], reference model.py:34-44, with the producer's
 *     BN+ReLU6 applied on load (bn may be NULL: input used as is).
 *   z[b,t,c] = sum_j w[j,c] * act(y[b, s*t + j - pad_l, c])      (0 outside [0,L_in))
 * bwd (DepthwiseConv2dNativeBackpropInput/Filter + ReluGrad + the BatchNorm reduction, a15):
 *   g[b,u,c]  = relu6'(.) * sum_j w[j,c] dz[b,(u+pad_l-j)/s,c]
 *   part      = per-block partial sums of (g, g*xhat, dw0, dw1, dw2), finalised by kws_dw_bwd_finalize.
 * ---------------------------------------------------------------------------------------- */
int kws_dwconv_fwd_f32(const float* y, const float* bn, const float* w, float* z, int B, int L_in,
                       int L_out, int C, int stride, int pad_l, void* stream);
int64_t kws_dwconv_bwd_part_floats(int B, int L_in, int C);
int kws_dwconv_bwd_f32(const float* dz, const float* y, const float* bn, const float* w, float* g,
                       float* part, int B, int L_in, int L_out, int C, int stride, int pad_l,
                       void* stream);
/* The same backward with the consumer's BatchNorm backward fused in, without materialising g
 * (reference: the BatchNormalization + relu6 + DepthwiseConv2D backward chain of model.py:34-51):
 *   pass 1: part only (fold with kws_dw_bwd_finalize -> dw, dgamma, dbeta and coef = [c1 | c2]);
 *   pass 2: dy[b,u,c] = scale[c] * (g - c1[c] - xhat * c2[c]), g recomputed from the same operands
 *           (bit-identical to kws_dwconv_bwd_f32 followed by kws_bn_bwd_apply).  bn must not be NULL. */
int kws_dwconv_bwd_bn_f32(const float* dz, const float* y, const float* bn, const float* w,
                          const float* coef, float* dy, float* part, int pass, int B, int L_in,
                          int L_out, int C, int stride, int pad_l, void* stream);
/* reduces part -> dw[3,C] (may be NULL), dgamma[C], dbeta[C], and coef[2*C] = (c1, c2) used by
 * kws_bn_bwd_apply; n_parts = part floats / (5*C) */
int kws_dw_bwd_finalize(const float* part, int n_parts, int64_t count, int C, float* dw,
                        float* dgamma, float* dbeta, float* coef, float* scratch, void* stream);
/* dy = gamma*rstd*(g - c1 - xhat*c2), in place on g (BatchNorm backward through batch stats) */
int kws_bn_bwd_apply(float* g, const float* y, const float* bn, const float* gamma,
                     const float* coef, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * DepthwiseConv2D((1, k), strides=s) on [B,1,L,C] with any tap count and stride, reference model.py:34-44 as the raw-waveform
 * models call it (conv_1d_gru_model, model.py:470-512: k 63 / 31 / 15 / 7 / 5 / 8 at strides 16 / 4 / 4 / 4 / 2 / 1): the general
 * form of kws_dwconv_*.  Channels-last [B, L, C], kernel w [k, C], the producer's BN+ReLU6 applied on load (bn may be NULL: the
 * input is used as is, no gate, and the first two rows of a part block are zero).  Zero padding applies to the ACTIVATION.
 *   fwd   z[b,t,c] = sum_{j<k} w[j,c] * act(y[b, s*t + j - pad_l, c])      (0 outside [0, L_in))
 *   bwd   g[b,u,c] = relu6'(bn(y[b,u,c])) * sum over j with s | (u + pad_l - j) and 0 <= t = (u + pad_l - j)/s < L_out of
 *                    w[j,c] * dz[b,t,c].  Every element of g [B, L_in, C] is written once; rows no window reaches are exact 0.
 *         part     = kws_dwconvk_bwd_part_rows() blocks [2 + k][C] of (sum g, sum g*xhat, dw_0 .. dw_{k-1}),
 *                    dw_j = sum_{b,t} act(y[b, s*t + j - pad_l, c]) * dz[b,t,c]
 *   finalize       part -> dw [k, C] (may be NULL), dgamma, dbeta (may be NULL), coef [2C] = (c1 | c2) for kws_bn_bwd_apply
 *                  (may be NULL); count = B * L_in
 * Domain: 1 <= k <= 64, 1 <= s <= 16, 0 <= pad_l < k, s*(L_out-1) + k - pad_l <= L_in + (k-1), C = 1 or C % 4 == 0 with
 * C <= 1024.  No atomics: results are bit-identical from run to run.
 * kws_dwconvk_pw1_*: the pointwise convolution 1 -> N behind a one-channel depthwise layer (K = 1 is outside kws_gemm_nn_f32):
 *   fwd   y[m,n] = z[m] * p[n]; stats_part (may be NULL): kws_dwconvk_pw1_stats_rows(M) rows [2][N] of (sum y, sum y^2) for
 *         kws_bn_stats_finalize
 *   bwd   dz[m] = sum_n dy[m,n] * p[n], dp[n] = sum_m z[m] * dy[m,n] (fixed order); workspace >=
 *         kws_dwconvk_pw1_bwd_workspace_floats(M, N) floats.  N: a power of two, 4 .. 256.
 * ---------------------------------------------------------------------------------------- */
int kws_dwconvk_fwd_f32(const float* y, const float* bn, const float* w, float* z, int B, int L_in, int L_out, int C,
                        int k, int stride, int pad_l, void* stream);
int kws_dwconvk_bwd_part_rows(int B, int L_in, int C, int k, int stride);
int64_t kws_dwconvk_bwd_part_floats(int B, int L_in, int C, int k, int stride);
int kws_dwconvk_bwd_f32(const float* dz, const float* y, const float* bn, const float* w, float* g, float* part, int B,
                        int L_in, int L_out, int C, int k, int stride, int pad_l, void* stream);
int kws_dwconvk_bwd_finalize(const float* part, int n_parts, int64_t count, int C, int k, float* dw, float* dgamma,
                             float* dbeta, float* coef, void* stream);
int kws_dwconvk_pw1_stats_rows(int64_t M);
int kws_dwconvk_pw1_fwd_f32(const float* z, const float* p, float* y, int64_t M, int N, float* stats_part, void* stream);
int64_t kws_dwconvk_pw1_bwd_workspace_floats(int64_t M, int N);
int kws_dwconvk_pw1_bwd_f32(const float* dy, const float* z, const float* p, float* dz, float* dp, int64_t M, int N,
                            float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The first _depthwise_conv_block of a narrow raw-waveform view (conv_1d_multi_time_sliced_model, model.py:1105-1140: the samples
 * as [4000, 4], [3200, 5], [640, 25]): DepthwiseConv2D((1, 3), VALID, stride 1) and the pointwise Conv1D(N, 1) in ONE kernel, for
 * channel counts outside kws_dwconvk_* and the GEMMs.  x [B, L, C] (the raw input, used as is), w [3, C], p [C, N]; C = 1 .. 32,
 * N % 4 == 0 with N <= 64, L >= 3.  The depthwise output is never written; the backward recomputes it.
 *   fwd   y[b,t,n] = sum_c p[c,n] * (sum_{j<3} w[j,c] * x[b,t+j,c]), t < L - 2; stats_part (may be NULL): kws_stem_stats_rows(B, L)
 *         rows [2][N] of (sum y, sum y^2) for kws_bn_stats_finalize
 *   bwd   dp[c,n] = sum_{b,t} z[b,t,c] * dy[b,t,n], dw[j,c] = sum_{b,t} x[b,t+j,c] * sum_n dy[b,t,n] p[c,n] (fixed-order partial rows
 *         and a fold: bit-identical from run to run); workspace >= kws_stem_bwd_workspace_floats(B, L, C, N) floats.  No gradient
 *         leaves the input.
 * ---------------------------------------------------------------------------------------- */
int kws_stem_stats_rows(int B, int L);
int kws_stem_fwd_f32(const float* x, const float* w, const float* p, float* y, int B, int L, int C, int N, float* stats_part,
                     void* stream);
int64_t kws_stem_bwd_workspace_floats(int B, int L, int C, int N);
int kws_stem_bwd_f32(const float* dy, const float* x, const float* w, const float* p, float* dw, float* dp, int B, int L, int C,
                     int N, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bidirectional(GRU(H, dropout, recurrent_dropout)) of Keras 2.1.2 (GRUCell, implementation=1, return_sequences=False,
 * merge_mode='concat'), reference model.py:148 (conv_1d_simple_model) and the GRU of xception_with_attention.  Per direction d
 * (0: t = 0 .. T-1, 1: t = T-1 .. 0, h = 0 before the first step), gates g in (z, r, h) = column blocks of kernel [I, 3H]:
 *   a_g = (x * mx_g) W_g + bias_g;  z = hs(a_z + (h * mh_z) U_z);  r = hs(a_r + (h * mh_r) U_r);  hs(v) = clip(0.2 v + 0.5, 0, 1)
 *   c = tanh(a_h + (r * h * mh_h) U_h)  (r before the product);  h' = z h + (1 - z) c;  out [B, 2H] = [h_fwd(T-1) | h_bwd(0)]
 * x [B, T, I]; W_d [I, 3H], U_d [H, 3H], bias_d [3H]; mx [2][3][B][I] and mh [2][3][B][H] hold 0 or 1 / keep per batch row (either
 * may be NULL: no mask).  kws_gru_masks draws them from the counter RNG of kws_dropout_fwd: layer id 16 + 6 d + g for mx_g and
 * 16 + 6 d + 3 + g for mh_g, element counter (row_offset + b) * n + i.
 *   kws_gru_seq_fwd_f32  the recurrence alone, ONE launch for all steps and both directions.  Pre-activation (d, g, b, t, j) is
 *                        read at a + d * dir_stride + g * gate_stride + (b * T + t) * row_stride + j (bias NOT included).  save
 *                        (NULL in inference): kws_gru_save_floats() floats [2][4: z, r, c, h][B, T, H].
 *   kws_gru_seq_bwd_f32  the same against time.  UT [2][3][H][H] with UT[d][g][k][j] = U_d[j][g H + k]; writes the pre-activation
 *                        gradients da [2][3][B T][H] (gate-major) and the left operands of U, lop [2][3][B T][H] =
 *                        (h_prev mh_z | h_prev mh_r | r h_prev mh_h), whose products with da are the gradients of U.
 *   kws_gru_fwd_f32      input projections (kws_gemm_nn_f32: one [B T, I] x [I, 3H] product per direction without mx, one per
 *                        gate on the materialised masked views of x with it) + the recurrence.
 *   kws_gru_bwd_f32      recurrence backward + dW, dU (kws_gemm_tn_f32), dbias (fixed-order column sums) per direction and
 *                        dx = sum_{d,g} (da_g W_g^T) * mx_g (dx may be NULL).  workspace: kws_gru_workspace_floats(.., backward)
 *                        floats; the backward needs nothing the forward left in it but `save`.
 * Domain: B >= 1, 1 <= T <= 1024, H % 16 == 0 with 16 <= H <= 256, I % 4 == 0.  No atomics: bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int64_t kws_gru_save_floats(int B, int T, int H);
int64_t kws_gru_workspace_floats(int B, int T, int I, int H, int backward);
int kws_gru_masks(float* mx, float* mh, int B, int I, int H, float keep_prob, uint64_t seed, uint32_t step, int64_t row_offset,
                  void* stream);
int kws_gru_seq_fwd_f32(const float* a, int64_t dir_stride, int64_t gate_stride, int row_stride, const float* U0, const float* U1,
                        const float* bias0, const float* bias1, const float* mh, float* out, float* save, int B, int T, int H,
                        void* stream);
int kws_gru_seq_bwd_f32(const float* dout, const float* UT, const float* mh, const float* save, float* da, float* lop, int B, int T,
                        int H, void* stream);
int kws_gru_fwd_f32(const float* x, const float* W0, const float* U0, const float* bias0, const float* W1, const float* U1,
                    const float* bias1, const float* mx, const float* mh, float* out, float* save, float* workspace, int B, int T,
                    int I, int H, void* stream);
int kws_gru_bwd_f32(const float* dout, const float* x, const float* W0, const float* U0, const float* W1, const float* U1,
                    const float* mx, const float* mh, const float* save, float* dx, float* dW0, float* dU0, float* dbias0, float* dW1,
                    float* dU1, float* dbias1, float* workspace, int B, int T, int I, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention gate in front of a recurrent layer, reference model.py:973-975 (xception_with_attention):
 *   attention = _context_conv(x, 1, k, padding='same')  (DepthwiseConv2D((1, k)) -> Conv1D(1, 1) -> BatchNormalization -> relu6),
 *   attention = softmax(attention, axis=1) over TIME, y = x * attention.
 *   u[b,t]   = sum_c Wa[c] sum_j wa[j,c] x[b, t + j - pl, c]     pl = (k - 1) / 2 (Keras 'same'); taps outside [0, T) read 0
 *   table[4] = scale | shift | mean | rstd of the ONE BatchNorm channel: training != 0 from the batch statistics of all B T values
 *              of u (fixed-order sums, biased variance, eps 1e-3; mm / mv updated at momentum 0.99), else from mm / mv
 *   att[b,t] = softmax_t(relu6(scale u + shift));  y[b,t,c] = x[b,t,c] att[b,t]
 * x, y, dy, dx [B, T, C]; wa [k, C] (the depthwise kernel [1, k, C, 1]); Wa [C] (the pointwise kernel [1, C, 1]); gamma, beta, mm,
 * mv, dgamma, dbeta [1]; u, att [B, T] are kept for the backward pass.
 *   kws_attn_gate_bwd_f32: da = sum_c dy x -> softmax backward over t -> ReLU6 mask (0 < scale u + shift <= 6) -> BatchNorm
 *   backward (training != 0: with the two batch sums, per-clip partials folded in a fixed order; else the table is constant)
 *   -> du [B, T];  dx = dy att + sum_j du[b, t - j + pl] Wa[c] wa[j,c];  with S_j[c] = sum_{b,t} du[b,t] x[b, t + j - pl, c]
 *   (per-clip partial rows, fixed-order fold): dwa[j,c] = Wa[c] S_j[c], dWa[c] = sum_j wa[j,c] S_j[c].  dx and dy are distinct buffers.
 * workspace: kws_attn_gate_fwd_floats / kws_attn_gate_bwd_floats floats (host-side planners, 0 outside the domain); the
 * backward needs nothing the forward left in its workspace.
 * Domain: B >= 1, 1 <= T <= 128, C % 4 == 0 with 4 <= C <= 1024, k in {3, 5}.  No atomics: bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int64_t kws_attn_gate_fwd_floats(int B, int T, int C, int k);
int64_t kws_attn_gate_bwd_floats(int B, int T, int C, int k);
int kws_attn_gate_fwd_f32(const float* x, const float* wa, const float* Wa, const float* gamma, const float* beta, float* mm,
                          float* mv, float* u, float* table, float* att, float* y, float* workspace, int B, int T, int C, int k,
                          int training, void* stream);
int kws_attn_gate_bwd_f32(const float* dy, const float* x, const float* u, const float* att, const float* table, const float* wa,
                          const float* Wa, const float* gamma, float* dx, float* dwa, float* dWa, float* dgamma, float* dbeta,
                          float* workspace, int B, int T, int C, int k, int training, void* stream);

/* ------------------------------------------------------------------------------------------
 * a14  optimizers on one flat parameter buffer, reference model.py:834 (RMSprop(lr=1e-3)) and
 *      model.py:96,110 (SGD momentum); constants SURVEY D.5.  g_eff = grad*grad_scale + 2*l2[i]*p
 *      (l2[i] = per-element kernel_regularizer coefficient, 0 for BN/bias).
 *      kws_rmsprop_step and kws_adam_step move four elements per 16-byte access: p, grad, acc / m / v and l2 must be
 *      16-byte aligned (whole allocations are), any n; a misaligned pointer is KWS_E_INVALID before any launch.
 *      kws_sgd_momentum_step and kws_l2_loss take any float-aligned pointers.
 * ---------------------------------------------------------------------------------------- */
int kws_rmsprop_step(float* p, const float* grad, float* acc, const float* l2, int64_t n, float lr,
                     float rho, float eps, float grad_scale, void* stream);
int kws_sgd_momentum_step(float* p, const float* grad, float* vel, const float* l2, int64_t n,
                          float lr, float momentum, float grad_scale, void* stream);
/* Keras 2.1.2 Adam (reference model.py:153,251,306,403,464): m' = beta1*m + (1-beta1)*g, v' = beta2*v + (1-beta2)*g^2,
 * p' = p - lr_t*m'/(sqrt(v') + eps).  lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) with t = iterations + 1 is the CALLER's (one host
 * value per step); eps is added to the un-corrected sqrt(v'), which is not torch.optim.Adam's rule.  m and v: n floats each. */
int kws_adam_step(float* p, const float* grad, float* m, float* v, const float* l2, int64_t n, float lr_t,
                  float beta1, float beta2, float eps, float grad_scale, void* stream);
/* out[0] = sum_i l2[i]*p[i]^2 (Keras regularisation loss) */
int kws_l2_loss(const float* p, const float* l2, int64_t n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Network programs: the whole forward / forward+backward of one model as a sequence of the
 * kernels above, launched natively (no Python between layers).
 *   KWS_NET_TS_ATTENTION: conv_1d_time_sliced_with_attention_model, reference model.py:775-838
 *   KWS_NET_LOG_MFCC:     conv_1d_log_mfcc_model, reference model.py:1400-1479 (and conv_1d_spectrogram_model,
 *                         model.py:1482-1561: num_features = 257)
 *   KWS_NET_STEFFE:       steffeNet, reference model.py:1663-1726 (raw input; input_size and num_classes only)
 *   KWS_NET_RESIDUAL:     conv_1d_residual_model, reference model.py:841-908 (raw input; filter_mult honoured)
 *   KWS_NET_MFCC_AND_RAW: conv_1d_mfcc_and_raw_model, reference model.py:1563-1660; the two Keras inputs arrive as ONE
 *                         row [mfcc spectrogram_length*num_features | raw samples], input_size = the row length
 *   KWS_NET_CONV_1D_FAST: conv_1d_fast_model, reference model.py:642-713 (raw input; Keras model name 'conv_1d_learned_spec')
 *   KWS_NET_CONV_1D_SPEC: conv_1d_spec_model, reference model.py:1249-1323 (input: the 'spec' output, fixed [98 * 257];
 *                         input_size is ignored).  Both: grouped Conv1D blocks (kws_gconv_*), each group its own Conv1D and
 *                         BatchNormalization layer; kws_net_debug_view what 0 = pre-BN output of conv layer `index` (0 = the
 *                         first, per grouped BLOCK: the groups concatenated [B, Lout, F]), what 2 = the table [4][Ng] of
 *                         batch_normalization_{index+1}.
 *   KWS_NET_CONV_1D_TIME_STACKED: conv_1d_time_stacked_model, reference model.py:257-309 (raw input, input_size must be 16000:
 *                         the reference reshapes to [800, 20])
 *   KWS_NET_CONV_1D_HEAVY: conv_1d_heavy_model, reference model.py:409-467 (raw input as [1600, 10]; Keras model name
 *                         'conv_1d_time_stacked' too).  Both: a ladder of dense VALID Conv1D (kws_gconv_* with one group) +
 *                         BatchNormalization + relu6, every second layer followed by kws_pool3s2_*; debug views as for the
 *                         grouped nets (what 0 = raw output of conv1d_{index+1}, conv_1d_heavy's Conv1D(128, 5) head included;
 *                         what 2 = table of batch_normalization_{index+1}).
 *   KWS_NET_CONV_1D_GRU:  conv_1d_gru_model, reference model.py:470-512 (raw input, input_size must be 16000; Keras model name
 *                         'conv_1d_bigru'; no recurrent layer): six depthwise blocks of kws_dwconvk_* + pointwise convolution +
 *                         BatchNormalization + relu6 (SAME k 63 / 31 / 15 / 7 / 5 at strides 16 / 4 / 4 / 4 / 2, VALID k 8) ->
 *                         Flatten -> Dropout(.3) -> Dense(256) + relu6 -> Dropout(.3) -> Dense + softmax.  Debug views: what 0 =
 *                         raw pointwise output of block `index` (0 .. 5), what 1 = depthwise output of block `index`, what 2 =
 *                         table of batch_normalization_{index+1}, what 4 = the hidden Dense layer's output before its bias.
 *   KWS_NET_CONV_1D_MULTI_TIME_SLICED: conv_1d_multi_time_sliced_model, reference model.py:1080-1156 (raw input, input_size must
 *                         be 16000): the samples viewed as [4000, 4], [3200, 5] and [640, 25], each view a ladder of depthwise blocks
 *                         (k 3 VALID; a _reduce_conv adds kws_pool3s2_same_*), the first block of a view on kws_stem_*; five one-step
 *                         branch ends of 64 channels (two of them tapped off a tensor the ladder goes on from) concatenated ->
 *                         Dropout(.1) -> a one-tap depthwise block (128) -> Dropout(.1) -> Conv1D(num_classes, 1, softmax, bias).
 *                         32 blocks in the reference's creation order; debug views: what 0 = raw pointwise output of block `index`
 *                         (0 .. 31), what 2 = table of batch_normalization_{index+1}.
 *   KWS_NET_CONV_1D_SIMPLE: conv_1d_simple_model, reference model.py:116-156 (raw input, input_size must be 16000; Keras model
 *                         name 'conv_1d_time_stacked'): fourteen VALID depthwise blocks on the ladder of KWS_NET_CONV_1D_GRU (k 31 at
 *                         stride 16 on one channel, then k 3 at strides 1, 2, 1, ...; F = 32, 32, 64, 64 .. 224, 224) ending at
 *                         [B, 10, 224] -> Bidirectional(GRU(128, dropout=.2, recurrent_dropout=.2)) (kws_gru_*) -> Dense + softmax.
 *                         Debug views: what 0 / 1 / 2 as for KWS_NET_CONV_1D_GRU (block `index` 0 .. 13), what 5 = the GRU's saved
 *                         steps [2 directions][4: z, r, c, h][B, 10, 128] (training), what 6 = the GRU output [B, 256].
 *   KWS_NET_XCEPTION_ATTENTION: xception_with_attention_model, reference model.py:911-983 (raw input, input_size even and at least
 *                         4000; filter_mult 1 or 2): the stem and residual blocks of KWS_NET_RESIDUAL over the block list (128, 2),
 *                         (256, 2), 8 x (256, 1), (384, 2) -> [B, 50, 384] at 16000 samples -> the attention gate kws_attn_gate_*
 *                         (k 5) -> Bidirectional(GRU(192, dropout=.2, recurrent_dropout=.2)) (kws_gru_*) -> Dense + softmax.
 *                         Debug views: what 0 / 2 as for KWS_NET_RESIDUAL, what 3 = attention weights att [B, T], what 4 = attention
 *                         logits u [B, T], what 5 = the last block's output [B, T, C], what 6 = the gate's output [B, T, C], what 7
 *                         = the GRU's saved steps [2 directions][4: z, r, c, h][B, T, 192] (training), what 8 = the GRU output
 *                         [B, 384], what 9 = the attention BatchNorm's table [4] = scale | shift | mean | rstd.
 *   KWS_NET_INCEPTION_D1: conv_inception_d1_model, reference model.py:312-406 (raw input, input_size must be 16000; Keras model
 *                         name 'inception_d1'): the samples as [800, 20] -> Conv1D(32, 1) -> three stride-1 reduce (MaxPool1D(3, 2)
 *                         behind) / context pairs of 64, 128, 256 filters, k 3 VALID (kws_gconv_* with one group + kws_pool3s2_*) ->
 *                         [B, 93, 256] -> eight inception blocks (1x1(64) | 1x1(48) -> k3 dil 2 (64) | 1x1(64) -> k3 dil d (96) twice
 *                         | AveragePooling1D(3, 1, 'same') -> 1x1(32), all SAME, concatenated: kws_conv1d_* writing the slices of the
 *                         joined tensor, kws_avgpool3_same_*; d = 2, 2, 2, 1, 1, 1, 1, 1) with a reduce block (k3(192) + pool |
 *                         1x1(32) -> k3(48) -> k3(48) + pool | MaxPool1D(3, 2, 'same') of the input; kws_pool3s2_same_*, 496
 *                         channels) behind every second one: T = 93, 47, 24, 12, 6 -> Dropout(.2) -> Conv1D(num_classes, 6,
 *                         softmax, bias) over the 6 remaining steps.  80 Conv1D in the reference's creation order; debug views: what
 *                         0 = raw output of Conv1D `index` (0 .. 78): a column window of the tensor it was written into, from its
 *                         first to its last element (count = (rows - 1) * pitch + filters), what 2 = table of
 *                         batch_normalization_{index+1}: the same columns of that tensor's table, the rows scale | shift | mean |
 *                         rstd one pitch apart (count = 3 * pitch + filters), what 3 = geometry of Conv1D `index`: offset = row
 *                         pitch, count = filters.
 *   KWS_NET_CONV_2D_MOBILE: conv_2d_mobile_model, reference model.py:547-594 (mfcc input [98 * 40], input_size must be 3920; Keras
 *                         model name 'conv_2d_mobile'): Reshape [98, 40, 1] -> Preprocess (clip((x + 0.8) / 7, -5, 5), no gradient) ->
 *                         eight Conv2D(F, 3 x 3, SAME, bias) -> BatchNormalization -> relu6, F = 32, 32, 64, 64, 128, 128, 256, 256,
 *                         the odd-numbered ones at stride 2 (49 x 20, 25 x 10, 13 x 5, 7 x 3; kws_conv2d_*), Dropout(.05) behind every
 *                         pair -> GlobalAveragePooling2D -> Dropout(.1) -> Dense + softmax, categorical CE; SGD(1e-3, momentum .95).
 *   KWS_NET_CONV_2D_FAST: conv_2d_fast_model, reference model.py:597-639 (the same input; 'conv_2d_fast'): four Conv2D(SAME, bias) ->
 *                         BatchNormalization -> relu -> MaxPool2D() (kws_pool2x2_*): 16 x (11, 5) dilation (2, 1), 32 x (5, 3)
 *                         dilation (2, 1), 64 x (3, 3), 128 x (3, 3); 98 x 40 -> 49 x 20 -> 24 x 10 -> 12 x 5 -> 6 x 2 ->
 *                         GlobalAveragePooling2D -> Dense + softmax; SGD(1e-3, momentum .9).
 *                         Both: weights in Keras order conv2d_<n>/kernel [kh, kw, Cin, F], conv2d_<n>/bias, batch_normalization_<n>/...
 *                         The bias stands in front of a BatchNormalization: training leaves it out of the GEMM (it cancels; its
 *                         gradient is written as exact 0) but adds it to the batch mean that updates moving_mean; inference folds
 *                         it into the table's shift.  Dropout counters (kws_dropout_fwd's RNG, element (row_offset + b) * H*W*F +
 *                         i of the NHWC tensor): layer id 1 = the tail's Dropout(.1), ids 2 .. 5 = the four Dropout(.05) in model
 *                         order.  Debug views: what 0 = raw output of conv2d_{index+1} WITHOUT the bias [B, Hout, Wout, F], what 1 =
 *                         what that layer hands on where it is materialised (pooled / dropped / last activation [B, Ho, Wo, F];
 *                         count 0 where the next convolution applies the table on load), what 2 = table of
 *                         batch_normalization_{index+1} [4][F], what 3 = the preprocessed input [B, 98, 40].
 *   KWS_NET_CONV_1D_TIME_SLICED: conv_1d_time_sliced_model, reference model.py:716-772 (raw input, input_size % 4 == 0 and long
 *                         enough for every block to keep a row: 12000 and 16000 are, 8000 is not; filter_mult 1 or 2): the front end
 *                         of KWS_NET_TS_ATTENTION at 32 * filter_mult filters (kws_frame_conv_*) -> thirteen 3-tap depthwise blocks
 *                         (stride, filters / filter_mult) = (1, 64) (2, 128) (1, 128) (2, 192) (1, 192) (2, 256) (1, 256) (2, 320)
 *                         (1, 320) (2, 384) (1, 384) (2, 512) (1, 512), stride 2 SAME and stride 1 VALID -> [B, 3, 512 fm] at 16000
 *                         samples -> GlobalAveragePooling1D -> Dropout(.4) (kws_gap_drop_*) -> Dense(256 fm, no bias) -> relu6 ->
 *                         Dropout(.3) -> Dense + softmax (no bias), categorical CE.  Dropout layer ids 1 and 2 in model order.  Debug
 *                         views: what 0 / 1 / 2 as for KWS_NET_TS_ATTENTION (y and tables 0 .. 13, z 0 .. 12), what 4 = the hidden
 *                         Dense layer's output before relu6 [B, 256 fm].
 *   KWS_NET_CONV_1D_LEARNED_SPEC: conv_1d_learned_spec_model, reference model.py:1159-1246 (raw input, input_size even and at least
 *                         14402 = 91 rows of 160 samples; Keras model name 'conv_1d_learned_spec', which conv_1d_fast shares): six
 *                         Conv1D(40, k, strides=160, SAME, no bias, l2 1e-4), k = 479, 383, 319, 255, 191, 161, concatenated to
 *                         [ceil(input_size / 160), 240] with no BN and no activation (kws_fbank_conv_*) -> four grouped reduce (k 3,
 *                         stride 2, 3 groups) / context (k 3, 2 groups) pairs of 300 ... 480 filters; the first context block's groups
 *                         read 180 and 120 of 300 channels (two kws_conv1d_* column windows) -> Flatten -> Dropout(.3) -> Dense.
 *                         Debug views: what 0, index 0 = the front output [B, rows, 240], index i >= 1 = block i's pre-BN output;
 *                         what 2, index j = the table of batch_normalization_{j+1} (4 * Ng floats).
 *   KWS_NET_CONV_1D_TOP_DOWN: conv_1d_top_down_model, reference model.py:1326-1397 (raw input, input_size at least 14879 = 91 rows:
 *                         the fewest that leave the last block a row; Keras model name 'conv_1d_top_down'): Conv1D(480, 479,
 *                         strides=160, VALID, WITH bias; no BN, no activation, no l2 - the gathered GEMM of KWS_NET_CONV_1D_FAST, its
 *                         bias added on load by the first block) -> four grouped reduce (3 groups, stride 2) / context (2 groups) pairs
 *                         of depthwise-separable blocks, k 3 VALID, l2 1e-5: every group a DepthwiseConv2D((1, 3)) -> Conv1D(F / g, 1)
 *                         -> BatchNormalization -> relu6 of its own (kws_gdwconv_* for all groups' depthwise halves, kws_gconv_* with
 *                         k = 1 for the pointwise ones).  Reduce groups read slices of (480, 300 of 420, 360, 300) / 3 channels; the
 *                         context groups each read ALL channels (the reference hands them x, not the slice).  Filters 420, 420, 360,
 *                         360, 300, 300, 240, 240 -> Flatten -> Dropout(.05) -> Dense + softmax, categorical CE.  The front bias stands
 *                         in front of block 1's BatchNormalization on batch statistics (depthwise and 1x1 keep a constant a constant):
 *                         it cancels in a training step and its gradient is written as exact 0.  Debug views: what 0,
 *                         index 0 = the front output WITHOUT its bias [B, rows, 480], index i >= 1 = block i's pre-BN output; what 1,
 *                         index i >= 1 = block i's depthwise output [B, Lout, g * gs]; what 2, index j = the table of
 *                         batch_normalization_{j+1} (4 * Ng floats).
 * The net handle holds only the host-side layer table.  Parameters live in ONE flat f32 buffer
 * (trainable, Keras layer order) + one flat state buffer (BN moving mean/variance), both owned by
 * the caller; kws_net_tensor_info enumerates the Keras-named tensors inside them.
 * ---------------------------------------------------------------------------------------- */
#define KWS_NET_TS_ATTENTION 1
#define KWS_NET_LOG_MFCC 2
#define KWS_NET_STEFFE 3
#define KWS_NET_RESIDUAL 4
#define KWS_NET_MFCC_AND_RAW 5
#define KWS_NET_CONV_1D_FAST 6
#define KWS_NET_CONV_1D_SPEC 7
#define KWS_NET_CONV_1D_TIME_STACKED 8
#define KWS_NET_CONV_1D_HEAVY 9
#define KWS_NET_CONV_1D_GRU 10
#define KWS_NET_CONV_1D_MULTI_TIME_SLICED 11
#define KWS_NET_CONV_1D_SIMPLE 12
#define KWS_NET_XCEPTION_ATTENTION 13
#define KWS_NET_INCEPTION_D1 14
#define KWS_NET_CONV_2D_MOBILE 15
#define KWS_NET_CONV_2D_FAST 16
#define KWS_NET_CONV_1D_TIME_SLICED 17
#define KWS_NET_CONV_1D_LEARNED_SPEC 18
#define KWS_NET_CONV_1D_TOP_DOWN 19
typedef struct kws_net kws_net_t;
typedef struct {
  int kind;
  int num_classes;
  int filter_mult;        /* TS_ATTENTION, RESIDUAL, XCEPTION_ATTENTION, CONV_1D_TIME_SLICED */
  int input_size;         /* 16000 (raw) or spectrogram_length*num_features */
  int spectrogram_length; /* LOG_MFCC only */
  int num_features;       /* LOG_MFCC only */
} kws_net_config_t;
typedef struct {
  char name[64];
  int64_t offset; /* float offset inside the params (is_state=0) or state (is_state=1) buffer */
  int64_t size;
  int ndim;
  int64_t shape[4];
  int is_state;
  float l2;       /* kernel_regularizer coefficient (0 if none) */
  int fan_in, fan_out; /* Glorot fans, 0 for non-kernels */
  float init;     /* constant initial value for non-kernels */
} kws_tensor_info_t;

int kws_net_create(const kws_net_config_t* cfg, kws_net_t** net);
int kws_net_destroy(kws_net_t* net);
/* arithmetic / launch schedule of this handle's pointwise GEMMs: 0 = f32 MFMA (default, the product path; since round 4 a
 * layer's input-gradient and weight-gradient GEMMs go out as ONE launch), 1 = f32 MFMA with the two as separate launches (the
 * schedule of rounds 1 - 3, kept as the A/B reference: bit-identical results; every net kind), 2 = the fp16 x 2 A/B arm (raw-waveform
 * attention net; other kinds ignore it).  State of the handle, not of the process. */
int kws_net_get_gemm_mode(const kws_net_t* net);
int kws_net_set_gemm_mode(kws_net_t* net, int mode);
int64_t kws_net_num_params(const kws_net_t* net);
int64_t kws_net_num_state(const kws_net_t* net);
int kws_net_num_tensors(const kws_net_t* net);
int kws_net_tensor_info(const kws_net_t* net, int idx, kws_tensor_info_t* info);
int64_t kws_net_workspace_bytes(const kws_net_t* net, int max_batch, int training);
/* parity/debug view into a workspace laid out for (batch, training): what = 0 pre-BN conv output
 * y[index] (0 = conv1d_1 .. 11 = conv1d_12), 1 depthwise output z[index], 2 BN table of
 * batch_normalization_{index+1} (scale|shift|mean|rstd), 3 attention weights [B,T] (training). */
int kws_net_debug_view(const kws_net_t* net, int batch, int training, int what, int index,
                       int64_t* offset_floats, int64_t* count);
/* inference (K.learning_phase()=0): moving statistics, no dropout. probs [B, num_classes] */
int kws_net_predict(const kws_net_t* net, const float* params, const float* state, const float* x,
                    int B, float* probs, void* workspace, int64_t workspace_bytes, void* stream);
/* one train_on_batch minus the optimizer: forward with batch statistics + dropout, loss
 * (a13: utils.py:87-108 for TS_ATTENTION, categorical_crossentropy for LOG_MFCC), backward,
 * BN moving-average update of `state`.  grads: flat buffer laid out like params (data-loss
 * gradient only, scaled by 1/loss_batch; L2 is folded into the optimizer).
 * metrics (device float[4]): sum of per-sample data loss, number of correct argmax, 0, 0.
 * row_offset: global index of row 0 (dropout counter offset for data-parallel shards). */
int kws_net_train_fwd_bwd(const kws_net_t* net, const float* params, float* state, const float* x,
                          const float* y_onehot, int B, float* grads, float* probs, float* metrics,
                          uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* The same step in two calls, so that the caller can start the gradient all-reduce of the LATE layers while the early
 * layers' backward still runs ("one fused buffer, overlapped with the tail of backward"; raw-waveform
 * attention net only):
 *   part 1  forward, classifier tail, backward of blocks n_blocks-1 .. split_block;
 *   part 2  backward of blocks split_block-1 .. 0 and of the first convolution.
 * After part 1 every gradient from float offset kws_net_grad_ready_offset(net, split_block) to the end of the flat
 * buffer is final.  Parts 1 + 2 enqueue exactly the launches of kws_net_train_fwd_bwd in the same order: the result is
 * bit-identical.  1 <= split_block < kws_net_num_blocks(net). */
int kws_net_num_blocks(const kws_net_t* net);
int64_t kws_net_grad_ready_offset(const kws_net_t* net, int split_block);
int kws_net_train_fwd_bwd_part(const kws_net_t* net, const float* params, float* state, const float* x,
                               const float* y_onehot, int B, float* grads, float* probs, float* metrics,
                               uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch,
                               void* workspace, int64_t workspace_bytes, int part, int split_block,
                               void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* KWS_HIP_H_ */
