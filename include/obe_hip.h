/*
 * obe_hip.h — C ABI of libobe_hip.so: the MI355X (gfx950) hot path of optbayesexpt.
 *
 * The reference (usnistgov/optbayesexpt 1.2.0) is pure Python + NumPy and has no
 * FFI of its own, so every entry point below names the reference *method* whose
 * arithmetic it replaces (paths relative to the reference root).  INTEGRATION.md
 * shows the ctypes stubs a maintainer of the reference would add.
 *
 * Conventions
 *  - All arithmetic is IEEE float64; indices are int64.
 *  - Every pointer named d_* is a DEVICE pointer owned by the caller (the Python
 *    host side allocates them as torch tensors); the library never allocates or
 *    frees device memory.  h_* are HOST pointers.  Result scalars (h_best, h_out, ...) may be
 *    pageable or page-locked: into page-locked memory (hipHostMalloc / hipHostRegister) the last
 *    kernel of the call writes them itself, otherwise they arrive by a small device-to-host copy.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *    kernels are enqueued on it; functions that return host scalars say so and
 *    synchronise that stream themselves.
 *  - Return value: 0 = success, otherwise a hipError_t (or -1 for an argument
 *    error); obe_last_error() describes the most recent failure on this thread.
 *  - No exceptions cross the ABI.  A handle-free, re-entrant design: all state
 *    lives in caller-owned buffers; calls on different streams are independent.
 *  - Particles are stored SoA: row i of `d_particles` (parameter i of every
 *    particle) starts at d_particles + i * ld_p   (particlepdf.py:101-105).
 *    Settings likewise: row k of `d_settings` at d_settings + k * ld_s
 *    (obe_base.py:174-176, meshgrid 'ij' flattened).
 */
#ifndef OBE_HIP_H
#define OBE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The only symbols the library (and every per-model plugin) exports: everything else is compiled with
 * -fvisibility=hidden (optbayesexpt_amd/build.py), tests/test_capi_symbols.py checks `nm -D` against this header. */
#define OBE_API __attribute__((visibility("default")))

/* 2 (round 6): obe_resample_begin gained d_aos; the sweep / arg-max calls write a 32-byte record into the
 * workspace tail and the speculative pair keeps its abort word there (OBE_WS_RESULT_TAIL, OBE_WS_ABORT_WORD);
 * limits raised.  3: two off-by-default entry points removed (the one-launch update's switch, the randoms enqueued
 * ahead of a resample); obe_resample_begin refuses a NULL h_pcg_state4.  A client compiled against another version must not call in: compare obe_abi_version(). */
#define OBE_ABI_VERSION 3
#define OBE_MAX_CONSTS 8
#define OBE_MAX_CHANNELS 8   /* output channels of a device model / of one measurement record */
#define OBE_MAX_SETDIMS 8    /* setting dimensions of a device model */
#define OBE_MAX_DIMS 32      /* parameter rows a device model may be given (obe_model.n_params) */
/* Up to OBE_FAST_DIMS parameter rows the cloud kernels (moments, the fused update, the pipelined resample) are
 * compiled for the exact row count, all accumulators in registers.  The calls that work on the cloud alone —
 * obe_moments, obe_resample_particles, obe_gather_columns, the masks, the unfused updates — take ANY number of rows
 * (the reference has no limit: particlepdf.py:105): beyond OBE_FAST_DIMS they run tiled over 8 rows at a time (one
 * pass over the cloud per tile, per tile pair for the covariance).  The fused / pipelined forms
 * (obe_bayes_update_model_moments*, obe_resample_begin, obe_resample_particles_aos*, obe_mask_renorm_moments)
 * refuse more than OBE_FAST_DIMS rows before anything is launched (-1); callers then use the plain forms. */
#define OBE_FAST_DIMS 16
#define OBE_CLOUD_MAX_DIMS 1024

/* ---- device model registry (replaces the Python `model_function` callable,
 *      obe_base.py:50-72, for the model families the reference's demos use) ---- */
enum obe_model_id {
    OBE_MODEL_LORENTZ = 1,      /* y = b + sum_k a/(((x-x0_k)/d)^2+1); aux = #peaks K (1..8);
                                   params x0_1..x0_K, a, b [, extras]; const d.
                                   K=1: demos/find_peak/sequentialLorentzian.py:53-75,
                                   demos/sweeper/sweeper.py:42-64                     */
    OBE_MODEL_LINE_AB = 2,      /* y = p0 + p1*x          tests/test_optbayesexpt.py:11-14 */
    OBE_MODEL_LINE_MB = 3,      /* y = p0*x + p1          demos/line_plus_noise/line_plus_noise.py:36-53 */
    OBE_MODEL_FIRST_PARAM = 4,  /* y = p0                 tests/test_zinference.py:21-26 */
    OBE_MODEL_RABI = 5,         /* demos/pipulse/pipulse.py:18-49; 2 settings, 2 params, 3 consts */
    OBE_MODEL_COIL = 6,         /* demos/lockin/lockin_of_coil.py:63-102; 2 channels */
    OBE_MODEL_PLUGIN = 100      /* a model generated from a user expression: served by its own
                                   plugin library (same entry points, compiled for that model) */
};

typedef struct obe_model {
    int32_t id;          /* enum obe_model_id */
    int32_t aux;         /* model-specific integer (number of Lorentzian peaks) */
    int32_t n_params;    /* D: rows of the particle array (may exceed what the model reads) */
    int32_t n_setdims;   /* S */
    int32_t n_channels;  /* C */
    int32_t n_consts;
    double consts[OBE_MAX_CONSTS];
} obe_model;

/* Checks id/aux/n_* consistency; fills n_setdims/n_channels if they are 0. */
OBE_API int obe_model_validate(obe_model* m);

/* ---- library ---- */
OBE_API int obe_abi_version(void);
/* Hash of the kernel sources this binary was compiled from (optbayesexpt_amd/build.py); the
 * loader compares it with the sources next to it and refuses a stale library. */
OBE_API const char* obe_source_fingerprint(void);
OBE_API const char* obe_last_error(void);
/* Deferred host results (per calling thread).  While on, the entry points that deliver results
 * to host memory and would synchronise `stream` for it — obe_moments (h_out), obe_weight_cdf
 * (h_total), obe_ziggurat_normal (h_consumed[2]) — only enqueue the copy and return; the values
 * are valid once the caller has synchronised the stream (pass page-locked host memory, or the
 * copy itself blocks).  resample() uses it to keep the device busy while the host factorises the
 * covariance.  Returns the previous state. */
OBE_API int obe_defer_host_sync(int32_t on);
/* The address under which kernels of the current device reach a page-locked host buffer
 * (hipHostMalloc / hipHostRegister; fails for pageable memory).  A `d_*` output argument that is
 * only a few values — the index of obe_draw_indices for good_setting() — may be given as this
 * address: the kernel then delivers the result to the host itself, with no copy back. */
OBE_API int obe_host_device_pointer(const void* h_pinned, void** d_out);
/* Waiting for such results by watching them: obe_host_words_arm stores a bit pattern no result has
 * (0x7ff8c0dec0dec0de: a NaN payload / an impossible index) into EVERY 8-byte word of a page-locked result
 * block, the call whose kernels write those words is enqueued, and obe_host_words_wait spins until none of
 * the words carries the pattern any more (bounded: after 400 us it synchronises `stream` instead, which also
 * reports a kernel that failed).  An 8-byte store arrives whole, so no ordering between the kernel's stores
 * is relied upon — watching one "last" word behind a system-scope fence was not safe for blocks that span
 * several 128-byte lines ("Waiting for a result by watching it").  5.9 us per round trip
 * of a short kernel instead of 11.1 us through hipStreamSynchronize (tools/microbench_sync.hip).  The entry
 * points that deliver host results into page-locked memory (obe_sweep_utility, obe_utility_argmax,
 * obe_argmax, obe_bayes_update_*, obe_weight_sums) wait this way themselves; obe_resample_begin and
 * obe_mask_nonpositive_moments arm their result words and leave the waiting to the caller.
 * obe_host_word_arm / _wait: the same for a single word. */
OBE_API int obe_host_words_arm(void* h_pinned_words, int64_t n_words);
OBE_API int obe_host_words_wait(const void* h_pinned_words, int64_t n_words, void* stream);
OBE_API int obe_host_word_arm(void* h_pinned_word);
OBE_API int obe_host_word_wait(const void* h_pinned_word, void* stream);
/* Name, CU count and memory of the current device; returns 0 if a gfx950 device is current. */
OBE_API int obe_device_info(char* name, int name_len, int* n_cu, int64_t* hbm_bytes);

/* Scratch (device) bytes any call below may need for these sizes.  The sweep keeps its draws,
 * packed once per call, in the workspace: pass n_particles >= the number of draws of any sweep
 * (N_DRAWS may exceed the particle count).  A plugin library answers for its own model. */
OBE_API int64_t obe_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_dims);

/* ---- K2: Bayes update  (obe_base.py:385-394 eval_over_all_parameters + likelihood +
 *      particlepdf.py:136-139 _normalized_product + :243-244 N_eff) ------------------
 * Fused: y = model(setting; particle), L = prod_ch exp(-((y-y_meas)/sigma)^2/2)/sigma,
 * [L = L^choke], t = nan_to_num(w*L), w' = nan_to_num(t/sum t), in place in d_weights.
 * sigma per channel: h_sigma[ch] (known noise, obe_base.py:451-456) when
 * h_noise_rows == NULL, otherwise row h_noise_rows[ch] of the particle array
 * (OptBayesExptNoiseParameter.likelihood, obe_noiseparam.py:109-115).
 * n_lik_channels = number of channels entering the product (zip truncation,
 * obe_base.py:453-455).  choke: NaN = none (obe_base.py:458-459).
 * h_out[0] = sum t, h_out[1] = sum nan_to_num(w'^2)  (host; stream is synchronised). */
OBE_API int obe_bayes_update_model(const obe_model* m,
                           const double* d_particles, int64_t ld_p, int64_t n_particles,
                           double* d_weights,
                           const double* h_setting, const double* h_y_meas,
                           const double* h_sigma, const int32_t* h_noise_rows,
                           int32_t n_lik_channels, double choke,
                           void* d_ws, int64_t ws_bytes, double* h_out, void* stream);

/* obe_bayes_update_model followed by the first pass of obe_moments on the updated weights, with the
 * normalisation and the moment sums fused into one pass over the cloud (pdf_update() of
 * obe_base.py:340-399 + mean()/std() of particlepdf.py:173-214, which every caller's cycle asks for
 * next, and the sweep's per-setting shift).  d_moments receives the K3 block without the covariance
 * (layout of obe_moments, bit-identical to calling it afterwards); h_out (nullable; sync) receives
 * [0] = sum t, [1] = sum w'^2, [2 .. 2 + 2 + 4 n_params) = that block.  n_dims = m->n_params.
 * Two launches: the workgroup of the normalisation pass that finishes last folds everyone's partial sums
 * (write-through partials, an arrival counter the library keeps per stream).  The weights and the moments
 * are the bits of obe_bayes_update_model() + obe_moments(); h_out[1] is summed from this pass's own
 * workgroup partials (one per CU) and can differ from obe_bayes_update_model()'s h_out[1] in the last
 * few ulp — never in a resample decision over the experiments tested
 * (tests/test_gpu_units.py::test_fused_and_unfused_update_take_the_same_resample_decisions). */
OBE_API int obe_bayes_update_model_moments(const obe_model* m,
                                   const double* d_particles, int64_t ld_p, int64_t n_particles,
                                   double* d_weights,
                                   const double* h_setting, const double* h_y_meas,
                                   const double* h_sigma, const int32_t* h_noise_rows,
                                   int32_t n_lik_channels, double choke, double* d_moments,
                                   void* d_ws, int64_t ws_bytes, double* h_out, void* stream);

/* strict sums (per calling thread; returns the previous setting, on < 0 only asks): while on, the UNFUSED updates —
 * obe_bayes_update_model, obe_bayes_update_y, obe_bayes_update_lik — form sum t and sum nan_to_num(w'^2) in the order
 * in which np.sum adds a contiguous float64 vector (pairwise_sum: pieces of 8192, runs of <= 128 in eight interleaved
 * running sums, halves split at multiples of 8; restated in oracle/obe_oracle.py: numpy_pairwise_sum and pinned there
 * against np.sum for every length to 5000), by one workgroup: the normalised weights t / np.sum(t) and N_eff are then
 * the reference's BITS (particlepdf.py:136-139, 243-244; its own tests compare them with assert_array_equal,
 * tests/test_optbayesexpt.py:58-69) wherever t itself is.  Meant for small clouds (the host side switches it on up to
 * 4096 particles: tuning_parameters['strict_sums']); any size works, one workgroup's speed.  The fused forms
 * (obe_bayes_update_model_moments*) ignore it. */
OBE_API int obe_strict_sums(int32_t on);

/* The same update, enqueued only: returns without waiting.  h_pinned_out (page-locked, 5 + 4 n_params
 * doubles) is armed here and written by the update's last kernel: [0] sum t, [1] sum w'^2, [2..) the K3
 * first-moment block, and [4 + 4 n_params] = 1.0 if auto_resample != 0 and the resample test of
 * particlepdf.py:236-258 on sum w'^2 (N_eff < 0.1 N or N_eff / N < resample_threshold) says "resample",
 * else 0.0 — wait with obe_host_words_wait(h_pinned_out, 5 + 4 n_params, stream).  The same decision stays
 * on the device, in the LAST 8-byte word of the caller's workspace (OBE_WS_ABORT_WORD: d_ws + ws_bytes - 8,
 * ws_bytes a multiple of 8), for an obe_sweep_utility(OBE_SWEEP_SPECULATIVE) call enqueued next on this
 * stream WITH THE SAME d_ws AND ws_bytes, which hides the host round trip of the update behind the sweep
 * (the reference's cycle is update -> resample test -> next opt_setting: obe_base.py:340-399, 733-756).
 * The word belongs to whoever owns the workspace: updates of other objects on the same stream do not touch it.
 * Refused (-1) BEFORE anything is launched — the weights are untouched and the caller uses the synchronous
 * form — when h_pinned_out is not page-locked, when the workspace has no 16 spare bytes behind what the
 * update uses (obe_workspace_bytes() always leaves them), or when the library has no arrival counter for
 * the stream (device allocation failed; a full table of 256 streams per device hands its least recently
 * used entry on after a device synchronisation, so it never refuses). */
#define OBE_WS_ABORT_WORD(d_ws, ws_bytes) ((unsigned*)((char*)(d_ws) + ((ws_bytes) & ~(int64_t)7) - 8))
OBE_API int obe_bayes_update_model_moments_enqueue(const obe_model* m, const double* d_particles, int64_t ld_p,
                                           int64_t n_particles, double* d_weights, const double* h_setting,
                                           const double* h_y_meas, const double* h_sigma,
                                           const int32_t* h_noise_rows, int32_t n_lik_channels, double choke,
                                           double* d_moments, void* d_ws, int64_t ws_bytes, double* h_pinned_out,
                                           int32_t auto_resample, double resample_threshold, void* stream);
/* A whole sweep of measurements (demos/sweeper/obe_sweeper.py:86-100: one pdf_update per point,
 * each followed by the resample test of particlepdf.py:236-258) enqueued back to back, no
 * host round trip between the points.  h_settings (n_points, OBE_MAX_SETDIMS) and h_y_meas
 * (n_points, OBE_MAX_CHANNELS) row-major; sigma / noise rows / choke as obe_bayes_update_model.
 * With auto_resample != 0 the test runs on the device after every point (in the prologue of
 * the next point's first pass: two launches per point): as soon as n_eff < 0.1 N or
 * n_eff / N < resample_threshold the remaining points are skipped (their kernels return at once).  h_out[0] = sum t and h_out[1] = sum w'^2 of the last point applied,
 * h_out[2] = 1 if a resample is due, h_out[3] = points applied (>= 1); the caller resamples and
 * submits the rest.  Sync. */
OBE_API int obe_bayes_update_sweep(const obe_model* m, const double* d_particles, int64_t ld_p,
                           int64_t n_particles, double* d_weights, const double* h_settings,
                           const double* h_y_meas, const double* h_sigma,
                           const int32_t* h_noise_rows, int32_t n_lik_channels, double choke,
                           int64_t n_points, int32_t auto_resample, double resample_threshold,
                           void* d_ws, int64_t ws_bytes, double* h_out, void* stream);
/* Same update from precomputed model outputs d_y (C, N_p) row-major, ld_y between
 * channels  (pdf_update(..., y_model_data), obe_base.py:384-385). */
OBE_API int obe_bayes_update_y(const double* d_y, int64_t ld_y, int32_t n_channels,
                       const double* d_particles, int64_t ld_p, int64_t n_particles,
                       double* d_weights, const double* h_y_meas,
                       const double* h_sigma, const int32_t* h_noise_rows,
                       int32_t n_lik_channels, double choke,
                       void* d_ws, int64_t ws_bytes, double* h_out, void* stream);

/* ParticlePDF.bayesian_update(likelihood) with a caller-supplied likelihood array
 * (particlepdf.py:216-234). */
OBE_API int obe_bayes_update_lik(const double* d_lik, int64_t n_particles, double* d_weights,
                         void* d_ws, int64_t ws_bytes, double* h_out, void* stream);

/* OptBayesExpt.likelihood(y_model, record) as an array (obe_base.py:418-461).  ANY number of channels (the
 * reference has no limit, obe_base.py:807-824): h_y_meas / h_sigma / h_noise_rows then hold n_lik_channels values
 * and a record wider than OBE_MAX_CHANNELS is multiplied up in groups of that many, in channel order, the choke
 * applied to the finished product. */
OBE_API int obe_likelihood_y(const double* d_y, int64_t ld_y, int32_t n_channels,
                     const double* d_particles, int64_t ld_p, int64_t n_particles,
                     const double* h_y_meas, const double* h_sigma,
                     const int32_t* h_noise_rows, int32_t n_lik_channels, double choke,
                     double* d_lik_out, void* stream);

/* h_out[0] = sum nan_to_num(w^2) (resample_test, particlepdf.py:243-244), h_out[1] = sum w. */
OBE_API int obe_weight_sums(const double* d_weights, int64_t n_particles,
                    void* d_ws, int64_t ws_bytes, double* h_out, void* stream);

/* ---- model evaluation wrappers (obe_base.py:298-338) ---- */
/* d_y_out (C, N_p): model(one setting; all particles). */
OBE_API int obe_eval_over_particles(const obe_model* m, const double* d_particles, int64_t ld_p,
                            int64_t n_particles, const double* h_setting,
                            double* d_y_out, int64_t ld_y, void* stream);
/* d_y_out (C, N_s): model(all settings; one parameter set h_params[D]). */
OBE_API int obe_eval_over_settings(const obe_model* m, const double* d_settings, int64_t ld_s,
                           int64_t n_settings, const double* h_params,
                           double* d_y_out, int64_t ld_y, void* stream);

/* ---- K3: weighted moments (particlepdf.py:173-214) ----
 * d_out layout (doubles): [0]=sum w, [1]=sum w^2, [2..2+D) mean (np.average),
 * [2+D..2+2D) m1 = sum w x, [2+2D..2+3D) m2 = sum w x^2, [2+3D..2+4D) std,
 * then (if want_cov) D*D covariance (np.cov aweights, ddof=1 form).  Stays on the
 * device (other kernels consume it); copied to h_out too when h_out != NULL (sync).
 * want_cov = 2: d_out already holds the first moments of these particles and weights (from an earlier
 * call or from obe_bayes_update_model_moments): only the covariance pass runs, about the mean found
 * there; of h_out only the covariance part is then written by a page-locked delivery. */
OBE_API int64_t obe_moments_len(int32_t n_dims);
OBE_API int obe_moments(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                const double* d_weights, int32_t want_cov,
                double* d_out, double* h_out, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- K4: multinomial resampling (particlepdf.py:260-345) ----
 * CDF of Generator.choice: cumsum(w) / cumsum(w)[-1].  strict_order != 0 reproduces
 * np.cumsum's serial rounding bit for bit (slow, one wavefront); 0 = parallel
 * blocked scan (same value to ~1e-13, indices identical unless a uniform falls
 * inside that gap).  h_total (nullable) receives what numpy validates of p (sync): sum(w) — NaN if any
 * weight is NaN — or -inf when some weight is negative ("Probabilities are not non-negative"). */
OBE_API int obe_weight_cdf(const double* d_weights, int64_t n_particles, int32_t strict_order,
                   double* d_cdf, double* h_total, void* d_ws, int64_t ws_bytes, void* stream);
/* ---- sweeper composition (demos/sweeper/obe_sweeper.py:122-149) ----
 * obe_cumsum: out = np.cumsum(x) (strict_order as above; no normalisation).
 * obe_interval_utility: utility[i] = (cum[stop_i] - cum[start_i]) / cost_i for the
 * n_pairs (start, stop) index rows of d_pairs (int64, row-major (n_pairs, 2)) — the
 * `(ends[:, 1] - ends[:, 0]) / cost` of sweep_utility(); cost_i = d_cost[i], or
 * stop_i - start_i + cost_of_new_sweep (sweep_cost_estimate(), obe_sweeper.py:106-120)
 * when d_cost == NULL.  Follow with obe_argmax. */
OBE_API int obe_cumsum(const double* d_x, int64_t n, int32_t strict_order, double* d_out,
               void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_interval_utility(const double* d_cum, int64_t n_settings, const int64_t* d_pairs,
                         int64_t n_pairs, const double* d_cost, double cost_of_new_sweep,
                         double* d_utility, void* stream);
/* The index part of randdraw() for a small draw (n_draws <= 64; the reference's N_DRAWS = 30,
 * good_setting's single draw): the uniforms travel as kernel arguments, the CDF is rebuilt
 * unless cdf_is_fresh (d_cdf still holds the CDF of d_weights), and for clouds of up to
 * 14 336 particles scan and search are one launch (beyond that the three-kernel scan is faster).  Same CDF bits and indices as
 * obe_weight_cdf + obe_cdf_search.  Never synchronises: when the CDF is rebuilt and
 * h_total_pinned != NULL (pinned host memory: written by the last kernel itself; pageable: an asynchronous copy), sum(w) lands there and is
 * valid after the caller's next synchronisation of the stream — or, for pinned memory, once the word itself has arrived: arm it with
 * obe_host_word_arm() before the call and wait for IT with obe_host_word_wait().  The arrival of another word (the indices copied
 * back, a later call's result) does not imply this one's: stores to host memory do not arrive in the order they were issued. */
OBE_API int obe_draw_indices(const double* d_weights, int64_t n_particles, int32_t strict_order,
                     int32_t cdf_is_fresh, double* d_cdf, const double* h_uniforms,
                     int32_t n_draws, int64_t* d_idx, double* h_total_pinned,
                     void* d_ws, int64_t ws_bytes, void* stream);
/* Systematic resampling (extension; BASELINE.json north_star names it, the reference itself is
 * multinomial): idx[i] = searchsorted(cdf, (i + u0) / n_draws, 'right') for ONE uniform u0 in
 * [0, 1).  Selected with tuning_parameters['resample_method'] = 'systematic'. */
OBE_API int obe_systematic_indices(const double* d_cdf, int64_t n, double u0, int64_t n_draws,
                           int64_t* d_idx_out, void* stream);
/* idx[j] = #{i : cdf[i] <= u[j]}  (searchsorted side='right'), int64.  d_ws (nullable): with at
 * least n / 2 + 8 bytes of scratch, a search of many draws (n_draws >= n / 4, n >= 32 768: a
 * resample) first builds a guide table of n / 8 + 1 bucket starts and then searches only the handful
 * of entries a draw's bucket spans — the same indices, ~3 instead of ~11 cold accesses per draw. */
OBE_API int obe_cdf_search(const double* d_cdf, int64_t n, const double* d_uniforms, int64_t n_draws,
                   int64_t* d_idx_out, void* d_ws, int64_t ws_bytes, void* stream);
/* randdraw gather: d_out (D, n_draws) = particles[:, idx]  (particlepdf.py:332-343).  An index outside
 * [0, n_particles) reads the nearest end of the cloud (particle 0 or n_particles - 1): nothing is read out of bounds. */
OBE_API int obe_gather_columns(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                       const int64_t* d_idx, int64_t n_draws,
                       double* d_out, int64_t ld_out, void* stream);
/* resample(): new[i,p] = old[i, idx[p]] + sum_j z[p,j] F[i,j]   (F = u*sqrt(s) of the
 * SVD of (1-a^2) cov, h_factor row-major D*D; z = standard normals (N, D) row-major);
 * if scale: new = new*a + mean[i]*(1-a)   (particlepdf.py:296-305).  Then weights = 1/N.
 * An idx[p] outside [0, n_particles) reads the nearest end of the cloud (particle 0 or n_particles - 1).
 * d_ws (nullable): with 8 * n_dims * n_particles bytes of scratch a large cloud is first copied
 * to (N, D) order, so that the gather of a particle touches one or two 64-byte sectors instead
 * of n_dims of them. */
OBE_API int obe_resample_particles(const double* d_old, int64_t ld_old, int32_t n_dims, int64_t n_particles,
                           const int64_t* d_idx, const double* d_normals,
                           const double* h_factor, const double* h_mean,
                           double a_param, int32_t scale,
                           double* d_new, int64_t ld_new, double* d_weights,
                           void* d_ws, int64_t ws_bytes, void* stream);
/* The same with the (N, D) copy of the old cloud already made (obe_resample_begin's d_aos): no copy pass in
 * front of the gather. */
OBE_API int obe_resample_particles_aos(const double* d_old_aos, int32_t n_dims, int64_t n_particles,
                               const int64_t* d_idx, const double* d_normals,
                               const double* h_factor, const double* h_mean,
                               double a_param, int32_t scale,
                               double* d_new, int64_t ld_new, double* d_weights, void* stream);

/* ... and with the first half of OptBayesExptNoiseParameter.enforce_parameter_constraints
 * (obe_noiseparam.py:57-79), which pdf_update() runs right after a resample, done by the gather: a new particle
 * whose parameter h_rows[k] <= 0 for any k gets weight 0 instead of 1/N, and d_mask_partials (2 x 2048 doubles,
 * the caller's) receives the partial sums {sum w, count} that obe_mask_nonpositive()'s first kernel would leave —
 * same grid, same order, same bits — for obe_mask_renorm_moments().  ONLY for a resample that the constraint
 * follows: the reference's resample() on its own leaves uniform weights.  This is
 * obe_resample_particles_aos_bounded with the bound (0, +inf) on the given rows (rows in [0, n_dims), at most
 * OBE_FAST_DIMS of them). */
OBE_API int obe_resample_particles_aos_masked(const double* d_old_aos, int32_t n_dims, int64_t n_particles,
                                      const int64_t* d_idx, const double* d_normals,
                                      const double* h_factor, const double* h_mean,
                                      double a_param, int32_t scale,
                                      double* d_new, int64_t ld_new, double* d_weights,
                                      const int32_t* h_rows, int32_t n_rows, double* d_mask_partials, void* stream);

/* The masked gather for declarative bounds on any parameter rows (OptBayesExpt.set_parameter_bounds; the hooks of
 * obe_noiseparam.py:57-79 and demos/lockin/lockin_of_coil.py:115-133 as data): a new particle whose row h_rows[k]
 * lies outside [h_lower[k], h_upper[k]] for any k — see obe_mask_bounds for h_open and the refusals, rows in
 * [0, n_dims) — gets weight 0 instead of 1/N.  d_mask_partials (2 x 2048 doubles, the caller's) receives the partial
 * sums {sum w, count} that obe_mask_bounds()'s first kernel would leave — same grid, same order, same bits — for
 * obe_mask_renorm_moments().  n_dims <= OBE_FAST_DIMS. */
OBE_API int obe_resample_particles_aos_bounded(const double* d_old_aos, int32_t n_dims, int64_t n_particles,
                                       const int64_t* d_idx, const double* d_normals,
                                       const double* h_factor, const double* h_mean,
                                       double a_param, int32_t scale,
                                       double* d_new, int64_t ld_new, double* d_weights,
                                       const int32_t* h_rows, const double* h_lower, const double* h_upper,
                                       const int32_t* h_open, int32_t n_rows, double* d_mask_partials, void* stream);

/* resample(), the device side up to the host's factorisation of the covariance, enqueued by ONE call
 * (particlepdf.py:260-301; RNG order as there: N uniforms for rng.choice, then N x D normals): the caller's
 * PCG64 stream continued on the device (h_pcg_state4 = {state hi, lo, increment hi, lo}; n_raw >= N + N D +
 * 4096 raw values are looked at, none is stored), the weight CDF into d_cdf (skipped when cdf_is_fresh), the N uniforms, the
 * search of the N draws (d_idx), the covariance of the PRE-resample cloud (have_first_moments: d_moments
 * already holds mean / std of these weights) and the N x D ziggurat normals (d_normals; d_zig_ws of
 * obe_ziggurat_workspace_bytes(n_raw - N) bytes).  Nothing is waited for.  Both host buffers must be
 * page-locked; every result word is armed here and the caller waits with obe_host_words_wait():
 *   h_f64[0]     sum(w) for numpy's validation of p (1.0, stored at once, when the CDF was fresh);
 *   h_f64[1..]   the K3 block: the covariance and, unless have_first_moments, the first moments — wait for
 *                the words h_f64 + 1 + lo .. h_f64 + 1 + obe_moments_len(D), lo = have_first ? 2 + 4 D : 0;
 *   h_i64[0..1]  {raw values the normals consumed, normals found}: wait for both, then obe_ziggurat_check().
 * d_aos (nullable, 8 n_dims N bytes): receives the (N, D) copy of the PRE-resample cloud for
 * obe_resample_particles_aos() — made here, while the host factorises, instead of in front of the gather; on
 * large clouds the covariance and this copy then run as a third chain beside the CDF / search and the random
 * numbers.  Same kernels, same numbers as the calls one by one. */
OBE_API int obe_resample_begin(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                       const double* d_weights, const uint64_t* h_pcg_state4, int32_t strict_cdf,
                       int32_t cdf_is_fresh, int32_t have_first_moments, int64_t n_raw,
                       double* d_cdf, double* d_uniforms, int64_t* d_idx, const void* d_zig_tables,
                       double* d_normals, void* d_zig_ws, int64_t zig_ws_bytes, double* d_moments,
                       double* h_f64, int64_t* h_i64, double* d_aos, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- K6: OptBayesExptNoiseParameter extras ----
 * enforce_parameter_constraints (obe_noiseparam.py:57-79): zero the weight of every
 * particle whose row h_rows[k] <= 0 for any k, renormalise if anything changed.
 * *h_changed = number of particles zeroed (sync).  obe_mask_nonpositive and obe_mask_nonpositive_moments are
 * obe_mask_bounds and obe_mask_bounds_moments (below) with the bound (0, +inf) on the given rows, under their own
 * argument checks. */
OBE_API int obe_mask_nonpositive(const double* d_particles, int64_t ld_p, int64_t n_particles,
                         const int32_t* h_rows, int32_t n_rows, double* d_weights,
                         int64_t* h_changed, void* d_ws, int64_t ws_bytes, void* stream);

/* The same mask AND the first moments of the constrained cloud (what obe_moments(want_cov = 0) would
 * compute next: every cycle needs them for the sweep's shift and the noise-parameter variance), bit for
 * bit, in two launches without a host round trip in between (obe_noiseparam.py:57-79 + particlepdf.py:
 * 173-214).  Does not wait: page-locked h_changed (1 word) and h_moments (the K3 block's 2 + 4 n_dims
 * first-moment values; either may be NULL) are armed here and written by the second kernel — the caller
 * waits with obe_host_words_wait() on each.  Pageable host buffers: the two calls above, synchronously. */
OBE_API int obe_mask_nonpositive_moments(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                                 const int32_t* h_rows, int32_t n_rows, double* d_weights, double* d_moments,
                                 double* h_moments, int64_t* h_changed, void* d_ws, int64_t ws_bytes,
                                 void* stream);

/* yvar_noise_model (obe_noiseparam.py:122-136): d_out[c] = weighted mean of
 * (particle row h_rows[c])^2, read from the K3 block: m2[row] / sum w.  No sync. */
/* The second half of obe_mask_nonpositive_moments() on its own — renormalise if anything was zeroed, first moments
 * of the constrained cloud, nothing waited for — from the partial sums a masked gather left in d_mask_partials
 * (obe_resample_particles_aos_masked).  Refused (-1) before any launch without an arrival counter for the stream or
 * with pageable host outputs: the caller then calls obe_mask_nonpositive_moments(), which on weights the gather has
 * already masked zeroes the same particles and leaves the same bits. */
OBE_API int obe_mask_renorm_moments(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                            const double* d_mask_partials, double* d_weights, double* d_moments,
                            double* h_moments, int64_t* h_changed, void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_noise_var_from_moments(const double* d_moments, int32_t n_dims, const int32_t* h_rows,
                               int32_t n_rows, double* d_out, void* stream);

/* ---- K6 for any rows: declarative parameter bounds (OptBayesExpt.set_parameter_bounds) ----
 * What the reference's users write as a NumPy hook — obe_noiseparam.py:57-79 (sigma <= 0), demos/lockin/
 * lockin_of_coil.py:115-133 (any parameter < 0) — as data: zero the weight of every particle whose row h_rows[k] is
 * below h_lower[k] or above h_upper[k] for any k, renormalise if anything changed.  h_open[k]: bit 0 = the lower
 * end is exclusive (a value EQUAL to h_lower[k] violates too), bit 1 = the upper end; an absent end is -inf / +inf
 * (its bit is ignored: a value of -inf / +inf never violates an absent end).
 * A NaN value violates nothing.  If every particle violates, the weights become NaN (0 / 0, as in NumPy and in
 * obe_mask_nonpositive).  Several entries may name one row: they intersect.  Model-independent.
 * Refused (-1) before anything is launched: a NULL pointer, n_rows outside 1..OBE_MAX_DIMS, a row outside
 * [0, OBE_CLOUD_MAX_DIMS) — [0, n_dims) where the call has n_dims —, a NaN bound, lower > upper, ld_p < n_particles.
 * *h_count = number of particles zeroed (sync).  (h_count / h_first_moments are obe_mask_nonpositive*'s h_changed /
 * h_moments: the delivery audit keeps its rules for these two calls in a table of their own, _audit._BOUNDS_RULES,
 * and reads the arguments by these names.) */
OBE_API int obe_mask_bounds(const double* d_particles, int64_t ld_p, int64_t n_particles,
                    const int32_t* h_rows, const double* h_lower, const double* h_upper, const int32_t* h_open,
                    int32_t n_rows, double* d_weights, int64_t* h_count, void* d_ws, int64_t ws_bytes,
                    void* stream);

/* The same mask AND the first moments of the constrained cloud, in two launches, nothing waited for: page-locked
 * h_count (1 word) and h_first_moments (2 + 4 n_dims values; either may be NULL) are armed here, as
 * obe_mask_nonpositive_moments arms its h_changed and h_moments, and the caller waits with obe_host_words_wait()
 * (obe_noiseparam.py:57-79, demos/lockin/lockin_of_coil.py:115-133 + particlepdf.py:173-214); pageable host buffers or more than
 * OBE_FAST_DIMS rows: obe_mask_bounds() + obe_moments(want_cov = 0), synchronously.  Bit for bit what those two
 * calls leave. */
OBE_API int obe_mask_bounds_moments(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                            const int32_t* h_rows, const double* h_lower, const double* h_upper,
                            const int32_t* h_open, int32_t n_rows, double* d_weights, double* d_moments,
                            double* h_first_moments, int64_t* h_count, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- parameter drift: the prediction step of the filter (ParticlePDF.drift; extension — the reference's parameters
 * are constants, its cloud moves only in the nudge of particlepdf.py:296-305) ----
 * n_rows chosen rows of the (D, N) cloud, h_rows ascending, do one step of a Gaussian random walk IN PLACE; the other
 * rows are never touched, nor are the columns n_particles .. ld_p of any row, nor the weights.  h_factor (n_rows x
 * n_rows, row-major) is G = sqrt(dt) L with L L^T the drift covariance per unit time, formed by the caller; d_normals
 * = standard normals (N, n_rows) row-major.  The contract is the chain itself, per drifted row k and particle p, every
 * operation one correctly rounded double operation:
 *   s = +0.0;  s = fma(z[p, j], G[k, j], s)  for j = 0 .. n_rows-1    (all n_rows terms, zeros of a triangular G too)
 *   v = x[h_rows[k], p] + s
 *   with h_lower / h_upper (n_rows each, the interval of row h_rows[k]; -inf / +inf: no bound there; both NULL: no
 *   reflection at all):  if v < lo: v = lo + (lo - v)  else if v > hi: v = hi - (v - hi)   — ONE reflection, each
 *   operation rounded on its own, a NaN left alone; a value still outside afterwards stays where it is (a mask's business)
 *   x[h_rows[k], p] = v
 * Nothing is waited for; no host result.  Model-independent.
 * Refused (-1) before anything is launched: a NULL pointer (h_lower and h_upper go together), n_rows outside
 * 1..OBE_FAST_DIMS, n_dims outside 1..OBE_CLOUD_MAX_DIMS, a row outside [0, n_dims), a row named twice or rows not
 * ascending, ld_p < n_particles, a factor entry that is not finite, a NaN bound, lower > upper. */
OBE_API int obe_drift_particles(double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                        const int32_t* h_rows, const double* h_factor, int32_t n_rows,
                        const double* d_normals, const double* h_lower, const double* h_upper, void* stream);

/* ---- good_setting (obe_base.py:781-784): p = nan_to_num(u ** exponent); p /= sum(p) ---- */
OBE_API int obe_power_normalize(const double* d_u, int64_t n, double exponent, double* d_p_out,
                        void* d_ws, int64_t ws_bytes, void* stream);

/* ---- K1 + K5: utility sweep and argmax (obe_base.py:463-489, 628-655, 733-756) ----
 * Evaluates the model over settings [s_begin, s_begin + n_settings) x draws and
 * reduces to the per-setting variance of the model output, per channel.
 *   d_draw_idx == NULL : full sweep — every particle is a draw, weighted variance
 *                        sum_p w_p (y - ybar)^2 / sum_p w_p     
 *   d_draw_idx != NULL : reference semantics — the n_draws listed particles, unweighted
 *                        ddof=0 variance (np.var over utility_y_space, obe_base.py:488)
 * d_moments: output of obe_moments for the same particles/weights (mean parameters are
 * used as the variance shift, sum w as the normaliser).
 * `shifted` is a bit set: OBE_SWEEP_SHIFTED (1), for expression (plugin) models
 * OBE_SWEEP_SAFE (2), and for the one-peak Lorentzian OBE_SWEEP_CELLS (4) and OBE_SWEEP_BINS (32; with
 * obe_sweep_utility_keep() also OBE_SWEEP_BINS_KEPT, 64).
 * OBE_SWEEP_SHIFTED set: moments are accumulated about a per-setting shift (always accurate).
 * OBE_SWEEP_SHIFTED clear: one instruction fewer per evaluation, accurate only while the predicted
 * mean does not dominate the spread; *h_kappa (nullable) returns the worst
 * (mean of y)^2 / var over settings and channels — the factor by which an unshifted sweep
 * amplifies rounding — so the caller can choose the mode for the next sweep, or repeat
 * this one with shifted = 1 if an unshifted result came back with a large factor.
 * Then utility[s] = sum_c yvar[c,s] / noise_var[c(,s)] / cost[(s)]   (obe_base.py:650-655)
 * with d_noise_var (C) if noise_ld == 0, (C, n_settings) rows noise_ld apart if noise_ld > 0, and, if
 * noise_ld = OBE_NOISE_FROM_MOMENTS(r0, r1, r2, r3) < 0, taken from the K3 block d_noise_var then points to
 * (obe_moments layout for m->n_params parameters; normally d_moments itself): channel c's noise variance is
 * that block's m2[r_c] / sum w — the weighted mean of sigma_c^2 of obe_noiseparam.py:122-136, the division
 * obe_noise_var_from_moments() does, without a launch of its own — and
 * cost = cost_scalar if d_cost == NULL else d_cost[s]; and the first-maximum argmax
 * (np.argmax, obe_base.py:748): h_best[0] = value, h_best_idx[0] = index relative to
 * s_begin (sync) when h_best != NULL.  d_yvar (C, n_settings) and d_utility
 * (n_settings) stay on the device. */
/* After obe_sweep_utility / obe_utility_argmax / obe_argmax the workspace holds the result
 * as one 32-byte record at d_ws + OBE_WS_RESULT_OFFSET doubles:
 * {best value (f64), best local index (i64 bits), kappa (f64), 0} — what a sharded caller
 * all-gathers across ranks (RCCL) without copying it to the host first. */
#define OBE_WS_RESULT_OFFSET 2
/* ... and once more in the last 48 bytes of the workspace, 4 doubles at d_ws + ws_bytes - 48 (ws_bytes a multiple
 * of 8; written when the workspace has that much room behind what the call uses — obe_workspace_bytes() always
 * leaves it): the update calls reuse the HEAD of the workspace, so a record that has to outlive them — the sweep
 * enqueued behind an update, whose record a sharded caller all-gathers one host round trip later — is read
 * there.  The word behind it is OBE_WS_ABORT_WORD. */
#define OBE_WS_RESULT_TAIL(d_ws, ws_bytes) ((double*)((char*)(d_ws) + ((ws_bytes) & ~(int64_t)7) - 48))
/* (5 bits per channel, channel c's row at bit 5 c, up to OBE_MAX_CHANNELS channels; rows below 32) */
#define OBE_NOISE_FROM_MOMENTS(r0, r1, r2, r3) \
    (-(int64_t)1 - ((int64_t)(r0) | ((int64_t)(r1) << 5) | ((int64_t)(r2) << 10) | ((int64_t)(r3) << 15)))
/* bits of the `shifted` argument of obe_sweep_utility / obe_sweep_kernel_time.  A plugin
 * model's fast sweep form batches its divisions without a branch and poisons (NaN) a batch
 * whose denominators leave the range in which that is exact; a NaN variance comes back as
 * *h_kappa = NaN, and the caller repeats the sweep with OBE_SWEEP_SAFE (one IEEE
 * reciprocal per element, implies the shift).  Of the built-in models the coil and the Lorentzian with 3
 * or more peaks have such a pair of forms; the latter's safe form still shares one reciprocal among the
 * 16 denominators of two particles x 8 settings of ONE peak and is exact for |x - x0| / d up to ~2e9
 * (tested to 2.5e7, tests/test_gpu_units.py::test_multi_peak_lorentzian_sweep_forms); the others ignore
 * OBE_SWEEP_SAFE.
 *
 * Completion of the "(sync)" entry points: the HOST results of a call are complete when it returns — they
 * are written by the call's last kernel into page-locked memory and waited for there — while device outputs
 * (weights, moments, utility ...) are ordered on the caller's stream like any kernel's: consume them on the
 * same stream, or synchronise it first.  obe_mask_nonpositive() in particular returns as soon as the count
 * is known, while the renormalisation it implies may still be running. */
#define OBE_SWEEP_SHIFTED 1
#define OBE_SWEEP_SAFE 2
/* OBE_SWEEP_SPECULATIVE (full sweeps only): the call is enqueued behind
 * obe_bayes_update_model_moments_enqueue() on the same stream, with the same d_ws and ws_bytes, and returns
 * at once.  Its kernels read the resample decision that update left in OBE_WS_ABORT_WORD(d_ws, ws_bytes) and
 * do nothing if it was "resample" (the cloud is about to change: particlepdf.py:236-258).  Refused (-1, before
 * any launch) if the workspace has no 16 spare bytes behind what the sweep uses.  Page-locked h_best / h_best_idx / h_kappa are armed, not waited
 * for: the caller first learns from the update's host block (word 4 + 4 n_params) whether the sweep ran,
 * and only then waits for the words with obe_host_words_wait().  An aborted call leaves them armed and the
 * device outputs (yvar, utility, the result record) untouched. */
#define OBE_SWEEP_SPECULATIVE 8
/* OBE_SWEEP_NOWAIT (full sweeps only): enqueued and not waited for, like OBE_SWEEP_SPECULATIVE, but
 * unconditional — the caller knows the cloud is final (after a resample) and collects the page-locked
 * result words later with obe_host_words_wait(). */
#define OBE_SWEEP_NOWAIT 16
/* OBE_SWEEP_CELLS: the one-peak Lorentzian's unshifted sweep summed by cell expansions (csrc/obe_models.h:
 * LorentzCells) instead of pair by pair — the setting axis x/d is cut into cells of half-width
 * 1 / OBE_CELL_RHO_INV, every particle adds OBE_CELL_ORDER Taylor coefficients of the two moments to each cell,
 * and a setting evaluates its cell's two polynomials.  The same moments to rounding (not the same bits), whatever
 * the order of the settings.  Ignored for every other model, with OBE_SWEEP_SHIFTED or OBE_SWEEP_SAFE, and for
 * the one-workgroup sweeps.  A call whose settings span more than OBE_CELL_MAX cells, hold a non-finite value, or
 * whose d is not finite and positive returns *h_kappa = NaN and NaN variances: the caller repeats it without the
 * bit.  obe_sweep_cells_plan() says beforehand whether a grid fits and whether the form pays. */
#define OBE_SWEEP_CELLS 4
#define OBE_CELL_RHO_INV 4
#define OBE_CELL_ORDER 28
#define OBE_CELL_MAX 128
/* the cell form is worth taking when the direct form's FP64 issue slots are at least this many times its own */
#define OBE_CELL_MIN_GAIN 2
/* Host only, nothing is launched: bit 0 — the cell form is valid for settings within [x_min, x_max] and the width d
 * (the span is within OBE_CELL_MAX cells, everything finite, d > 0); bit 1 — it is also worthwhile: n_settings
 * direct evaluations per particle cost at least OBE_CELL_MIN_GAIN times the issue slots of the cells' expansions,
 * and the sweep's n_draws draws (the particles, for a full sweep) are enough to fill the expansion kernel's grid. */
OBE_API int obe_sweep_cells_plan(double x_min, double x_max, double d, int64_t n_settings, int64_t n_draws);
/* OBE_SWEEP_BINS: the same sweep with the PARTICLES summarised instead of the settings (csrc/obe_models.h:
 * LorentzBins) — the packed positions x0/d are cut into bins of half-width 1 / OBE_CELL_RHO_INV, the draws are
 * grouped by bin (the order of a stable sort, so every sum has a fixed order: the same bits from call to call), each
 * bin keeps 3 OBE_CELL_ORDER moments of its draws about its centre, and a setting meets the occupied bins instead of
 * the draws.  Honoured where OBE_SWEEP_CELLS would be (it goes before that bit where both are set) for up to 2^30
 * draws; the same moments to rounding.  A call whose x0/d span more than OBE_BIN_MAX bins (zero-weight draws
 * included), hold a non-finite value, or whose d is not finite and positive returns *h_kappa = NaN and NaN
 * variances: the caller repeats it without the bit.  The span depends on the particles alone, so a caller need not
 * ask again before the cloud changes. */
#define OBE_SWEEP_BINS 32
#define OBE_BIN_MAX 128
/* Host only, nothing is launched: bit 0 — the inputs are finite and d > 0 (whether the cloud fits OBE_BIN_MAX bins
 * only the call itself finds out); bit 1 — the form is also worthwhile: priced at OBE_BIN_MAX occupied bins plus the
 * pass over the draws plus the fixed cost of its launches, the form it would replace (the cells where
 * obe_sweep_cells_plan() takes them, otherwise the direct kernel) costs at least OBE_CELL_MIN_GAIN times as much. */
OBE_API int obe_sweep_bins_plan(double x_min, double x_max, double d, int64_t n_settings, int64_t n_draws);
/* Host only, nothing is launched: the wavefronts that share each group of 64 settings when an OBE_SWEEP_BINS call of
 * n_settings settings (the call's own: a rank's slice) evaluates the bins — 8 up to 16 384 settings, 6 up to 32 768,
 * 3 up to 65 536, the largest at which every workgroup of the launch is resident at once, and 1 beyond.  The results
 * do not depend on it. */
OBE_API int obe_sweep_bins_eval_waves(int64_t n_settings);
/* Settings one lane of the sweep kernel owns at most for a grid of n_settings (1, 2, 4 or 8; a sweep of
 * few draws may use fewer): the number of denominators a model's fast form inverts together, which a
 * caller that predicts whether a settings grid stays inside that form's range needs
 * (optbayesexpt_amd/models.py: range_hint). */
OBE_API int obe_sweep_settings_per_lane(int64_t n_settings);
/* ... and for a reference-semantics sweep of n_draws draws (obe_base.py:463-489 with N_DRAWS draws): 1 when the
 * one-workgroup kernel serves it.  A model whose fast form shares nothing but the reciprocal of a lane's
 * settings is IEEE as it is when this returns 1: no range check, no repeat (models.py: safe_sweep_min_spt). */
OBE_API int obe_sweep_settings_per_lane_for(int64_t n_settings, int64_t n_draws);
OBE_API int obe_sweep_utility(const obe_model* m,
                      const double* d_settings, int64_t ld_s, int64_t n_settings,
                      const double* d_particles, int64_t ld_p, int64_t n_particles,
                      const double* d_weights, const int64_t* d_draw_idx, int64_t n_draws,
                      const double* d_moments, int32_t shifted,
                      const double* d_noise_var, int64_t noise_ld,
                      const double* d_cost, double cost_scalar,
                      double* d_yvar, double* d_utility,
                      double* h_best, int64_t* h_best_idx, double* h_kappa,
                      void* d_ws, int64_t ws_bytes, void* stream);
/* ---- the grouping of an OBE_SWEEP_BINS sweep, kept from one call to the next ----
 * Which bin a draw belongs to, where each bin's run of sorted draws starts and where every draw goes in that order
 * depend on the packed x0/d alone: not on the weights, the mean parameters or the settings.  The workspace is scratch
 * of every library call, so what is to outlive a sweep lives in a buffer the CALLER owns: device memory of at least
 * obe_sweep_bins_keep_bytes(n_particles) bytes, 16-byte aligned, used by one sweep at a time (a head of 16 ints, the
 * two tables of OBE_BIN_MAX + 2 ints and one int32 position per draw; host only, nothing is launched). */
OBE_API int64_t obe_sweep_bins_keep_bytes(int64_t n_draws);
/* The records form of the same buffer: obe_sweep_bins_keep_bytes(n) bytes as above, unchanged, and behind them, each
 * 16-byte aligned, the particle part of every draw in sorted order (24 bytes: x0/d, a, b) and a dense array of the
 * draws' sqrt(w) in the same order; at least obe_sweep_bins_keep_bytes(n) + 32 n bytes, a multiple of 16 (host only,
 * nothing is launched).  The keep_bytes of a call selects the form: a call that is told at least this size keeps the
 * draws' records in d_keep instead of the workspace, and says so in the head (the first of its seven pad words: the
 * only byte of the first obe_sweep_bins_keep_bytes(n) that differs from what a call told the smaller size leaves). */
OBE_API int64_t obe_sweep_bins_keep_records_bytes(int64_t n_draws);
/* OBE_SWEEP_BINS_KEPT (a bit of `shifted`): the caller says that d_keep was filled by an earlier call of
 * obe_sweep_utility_keep() with the same d_particles, ld_p, n_particles and d, and that no particle value has
 * changed since.  Honoured only together with OBE_SWEEP_BINS where that bit is, in a full sweep (d_draw_idx == NULL:
 * draws are drawn anew for every call) and with a d_keep of at least obe_sweep_bins_keep_bytes(n_particles) bytes;
 * otherwise ignored. */
#define OBE_SWEEP_BINS_KEPT 64
/* obe_sweep_utility() with a keep buffer behind its arguments (h_value, h_index, h_factor: its h_best, h_best_idx,
 * h_kappa); d_keep == NULL, a keep_bytes too small for the call, a draws-mode call or a call that does not take the
 * bin form: exactly obe_sweep_utility(), and d_keep is not touched.  Otherwise
 *   OBE_SWEEP_BINS_KEPT clear: the sweep of OBE_SWEEP_BINS, which leaves its plan, its tables and every draw's
 *     sorted position in d_keep and marks the buffer complete with its last grouping launch (a poisoned plan is kept
 *     as such; a speculative call that is aborted leaves the buffer as it was);
 *   OBE_SWEEP_BINS_KEPT set: the four grouping launches of a rebuild (it has no pack of its own: the last of them
 *     forms the records) are replaced by ONE launch that writes every draw's packed record straight to its kept
 *     position — the same records in the same places, so the same bits as a rebuild.  The caller's word alone decides
 *     nothing: every kernel first checks the head (complete, made for n_particles draws and this d), and that one
 *     launch checks of every draw that its x0/d is finite and still lies in the
 *     bin whose run holds its kept position.  A buffer that fails either check makes the call return *h_factor = NaN
 *     and NaN variances, as a poisoned plan does, and nothing is written through it: the caller repeats the call
 *     without the bit.  (A particle that moved within its bin passes, and gives what a rebuild gives.)
 *   OBE_SWEEP_BINS_KEPT set and keep_bytes >= obe_sweep_bins_keep_records_bytes(n_particles), the records form: the
 *     call RELIES on what the bit says, "no particle value has changed since".  That one launch writes only sqrt(w) of
 *     every draw to its kept position: it reads no particle and checks no bin, and the records are formed from the
 *     kept particle parts, the new weights and d_moments - the bits of a rebuild if the caller's word holds.  What
 *     is read and written through the buffer still rests on the head alone (the library wrote every position itself,
 *     and checks its range all the same); the validity of the RESULT rests on the caller's word, as it does for
 *     d_moments in every sweep: a changed particle gives the sweep of the old particles with the new weights,
 *     unspecified but finite.  A caller who wants every draw checked passes obe_sweep_bins_keep_bytes(n_particles).
 *     (A buffer whose last rebuild was told the smaller size has no records: the call takes the checking path.)
 * OBE_SWEEP_SPECULATIVE, OBE_SWEEP_NOWAIT, obe_sweep_timing() and the result records work as in obe_sweep_utility().
 * obe_sweep_kernel_time() has no keep buffer: it times the whole rebuild. */
OBE_API int obe_sweep_utility_keep(const obe_model* m,
                      const double* d_settings, int64_t ld_s, int64_t n_settings,
                      const double* d_particles, int64_t ld_p, int64_t n_particles,
                      const double* d_weights, const int64_t* d_draw_idx, int64_t n_draws,
                      const double* d_moments, int32_t shifted,
                      const double* d_noise_var, int64_t noise_ld,
                      const double* d_cost, double cost_scalar,
                      double* d_yvar, double* d_utility,
                      double* h_value, int64_t* h_index, double* h_factor,
                      void* d_ws, int64_t ws_bytes, void* stream,
                      void* d_keep, int64_t keep_bytes);

/* Variance over the draw axis of a caller-filled y-space (N_d, C, N_s) — the
 * np.var(utility_y_space, axis=0) of obe_base.py:488 for host-callable models. */
OBE_API int obe_yspace_variance(const double* d_yspace, int64_t n_draws, int32_t n_channels,
                        int64_t n_settings, double* d_yvar, void* stream);
/* utility + argmax from an existing yvar (same conventions as obe_sweep_utility). */
OBE_API int obe_utility_argmax(const double* d_yvar, int32_t n_channels, int64_t n_settings,
                       const double* d_noise_var, int64_t noise_ld,
                       const double* d_cost, double cost_scalar,
                       double* d_utility, double* h_best, int64_t* h_best_idx,
                       void* d_ws, int64_t ws_bytes, void* stream);
/* first-maximum argmax of an arbitrary device vector (np.argmax semantics incl. NaN). */
OBE_API int obe_argmax(const double* d_v, int64_t n, double* h_best, int64_t* h_best_idx,
               void* d_ws, int64_t ws_bytes, void* stream);

/* ---- the non-default utilities on the explicit y-space ----
 * d_yspace (N_d, C, N_s) row-major = utility_y_space of the reference (obe_base.py:293-295). */
/* y[d][c][s] = model(setting s; particle d_draw_idx[d]) — the loop of obe_base.py:483-484
 * (eval_over_all_settings per drawn parameter set), exact NumPy operation order. */
OBE_API int obe_eval_draws(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                   const double* d_particles, int64_t ld_p, int64_t n_particles,
                   const int64_t* d_draw_idx, int64_t n_draws, double* d_yspace, void* stream);
/* y[d][c][:] += d_noise[d][c]  (utility_full_kld, obe_base.py:714-715). */
OBE_API int obe_yspace_add_noise(double* d_yspace, int64_t n_draws, int32_t n_channels, int64_t n_settings,
                         const double* d_noise, void* stream);
/* yvar_max_min (obe_base.py:520-535): (max - min)^2 over the draws, per column (C*N_s columns). */
OBE_API int obe_yspace_maxmin(const double* d_yspace, int64_t n_draws, int64_t n_columns, double* d_span2, void* stream);
/* scipy.stats.differential_entropy(axis=0, method='auto') per column (obe_base.py:516, 717-718);
 * as_variance != 0 returns exp(2H)/(2 pi e) (yvar_from_entropy, obe_base.py:517).
 * d_scratch: n_draws * n_columns doubles.  n_draws <= 2048. */
OBE_API int obe_yspace_entropy(const double* d_yspace, int64_t n_draws, int64_t n_columns, int32_t as_variance,
                       double* d_scratch, double* d_out, void* stream);
/* utility_full_kld (obe_base.py:720): exp(H_y[c,s] - H_noise[c]) - 1. */
OBE_API int obe_kld_utility(const double* d_entropy_y, int32_t n_channels, int64_t n_settings,
                    const double* d_entropy_noise, double* d_utility, void* stream);

/* ---- device-side continuation of the caller's numpy PCG64 stream ----
 * Replaces the host calls inside resample(): rng.random(n) (the uniforms Generator.choice
 * draws, particlepdf.py:330) and rng.standard_normal((n, d)) (inside multivariate_normal,
 * particlepdf.py:300).  h_state4 = {state_hi, state_lo, inc_hi, inc_lo} of
 * rng.bit_generator.state; d_raw[i] = the (i+1)-th next_uint64 of that generator. */
OBE_API int obe_pcg64_raw(const uint64_t* h_state4, int64_t n_raw, uint64_t* d_raw, void* stream);
/* d_out[i] = (d_raw[i] >> 11) * 2^-53  (numpy next_double / Generator.random). */
OBE_API int obe_pcg64_uniform(const uint64_t* d_raw, int64_t n, double* d_out, void* stream);
/* The same draws without a buffer of raw values, in two stages (what obe_resample_begin enqueues): stage 1 —
 * ONE launch for the n_uniform uniforms of Generator.choice and the classification of the n_raw_normal raw
 * positions behind them, every thread carrying the generator state of its position (h_state4 as for
 * obe_pcg64_raw); stage 2 — start flags, scan and compaction of the first n normals into d_out, h_consumed as
 * for obe_ziggurat_normal.  d_ws of obe_ziggurat_workspace_bytes(n_raw_normal) bytes, the same for both. */
OBE_API int obe_pcg64_uniforms_classify(const uint64_t* h_state4, int64_t n_uniform, int64_t n_raw_normal,
                                double* d_uniforms, const void* d_tables, void* d_ws, int64_t ws_bytes,
                                void* stream);
OBE_API int obe_ziggurat_finish(int64_t n_raw_normal, int64_t n, double* d_out, int64_t* h_consumed, void* d_ws,
                        int64_t ws_bytes, void* stream);
/* n standard normals by numpy's ziggurat from d_raw[offset...]: bit-identical values and
 * the exact number of raw values consumed (*h_consumed; sync), so the host generator can
 * be advanced to where numpy would have left it.  d_tables = ki[256] (uint64) | wi[256] |
 * fi[256] (float64).  Returns 1 if n_raw is too short (retry with a longer buffer).
 * With obe_defer_host_sync on: h_consumed[0..1] receive {raw values consumed, normals found}
 * asynchronously and the return value only reports launch errors; after synchronising, the
 * caller checks them with obe_ziggurat_check (1 = buffer too short). */
OBE_API int64_t obe_ziggurat_workspace_bytes(int64_t n_raw);
OBE_API int obe_ziggurat_normal(const uint64_t* d_raw, int64_t n_raw, int64_t offset, const void* d_tables,
                        int64_t n, double* d_out, int64_t* h_consumed,
                        void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_ziggurat_check(int64_t consumed, int64_t found, int64_t n, int64_t n_raw, int64_t offset);

/* ---- posterior summaries: marginals, joint histograms, quantiles (extension) ----
 * What the reference's users read from the whole cloud after a cycle — the weighted scatter plots of
 * demos/pipulse/pipulse.py:159 and demos/find_peak/seqLor_pdfevolve.py:156-163, the histograms quoted in
 * docs/manual_demos.rst, the 95 % credible intervals tests/test_gpu_trajectories.py:186 argues with —, next to the
 * mean / covariance / std of particlepdf.py:173-214, without copying the cloud to the host.
 * Fixed point: every weight enters as the integer Q_i = rint(w_i 2^k), NaN and negative weights as 0, with
 * k = 62 - e for the smallest e with sum(w) <= 2^e (1 + 2^-20) (k = 62 for normalised weights; sum(Q) < 2^63).  Bins
 * and cumulative sums are unsigned 64-bit integers, so every result is the same bits from run to run and under any
 * permutation of the cloud; a mass is Q_bin 2^-k, within 4 eps mass + n_bin 2^-62 sum(w) of the exact sum.  Weights
 * must be finite.  All results land in the caller's DEVICE buffers, nothing is waited for.  h_rows: the n_rows
 * parameter rows (each in [0, n_dims)) the call serves; d_ws: obe_posterior_workspace_bytes(n_particles, n_rows,
 * bins per row — bins_x * bins_y with n_rows = 1 for the joint form —, n_q) bytes, a buffer of its own (the calls
 * use its head, where obe_workspace_bytes()'s workspace keeps other calls' results). */
OBE_API int64_t obe_posterior_workspace_bytes(int64_t n_particles, int32_t n_rows, int64_t n_bins, int32_t n_q);
/* d_minmax[2 r], d_minmax[2 r + 1] = np.min / np.max of row h_rows[r] over ALL particles (both NaN if the row holds
 * one; -0.0 reported as 0.0): the automatic range of np.histogram_bin_edges. */
OBE_API int obe_minmax_rows(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                    const int32_t* h_rows, int32_t n_rows, double* d_minmax, void* d_ws, int64_t ws_bytes,
                    void* stream);
/* d_mass (n_rows, n_bins) = np.histogram(particles[h_rows[r]], weights = w) over the caller's edges d_edges
 * (n_rows, n_bins + 1), ascending.  Membership is decided by the edge array alone: bin k holds
 * edges[k] <= x < edges[k + 1], the last bin also x == edges[n_bins]; values outside and NaN are not counted.  Up to
 * 4096 bins per row the bins of as many rows as fit are kept in 32 KiB of LDS per workgroup (one pass over the cloud
 * per group of rows); beyond, up to 2^24 bins per row, the adds go to global memory.  More is refused (-1). */
OBE_API int obe_weighted_histogram(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                           const double* d_weights, const int32_t* h_rows, int32_t n_rows, const double* d_edges,
                           int64_t n_bins, double* d_mass, void* d_ws, int64_t ws_bytes, void* stream);
/* d_mass (n_bins_x, n_bins_y) row-major = np.histogram2d(particles[row_x], particles[row_y], weights = w) over the
 * caller's edges, same membership rule per axis.  n_bins_x * n_bins_y <= 4096 in LDS, <= 2^24 at all. */
OBE_API int obe_weighted_histogram2d(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                             const double* d_weights, int32_t row_x, int32_t row_y, const double* d_xedges,
                             int64_t n_bins_x, const double* d_yedges, int64_t n_bins_y, double* d_mass,
                             void* d_ws, int64_t ws_bytes, void* stream);
/* d_quantiles (n_rows, n_q) = np.quantile(particles[h_rows[r]], h_q, weights = w, method = "inverted_cdf"): the
 * smallest particle value x with sum_{x_i <= x} Q_i >= max(1, ceil(q sum Q)), in np.sort's order (-0.0 == 0.0, NaN
 * last; NaN if every weight is zero).  A radix select on the 64-bit order-preserving key: 8 passes of 8 bits, each a
 * weighted digit histogram of the keys that carry the digits chosen so far, the digit chosen by a small kernel in
 * between; one call serves every row and up to 16 values of q (each in [0, 1]) with the same 8 passes. */
OBE_API int obe_weighted_quantiles(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                           const double* d_weights, const int32_t* h_rows, int32_t n_rows, const double* h_q,
                           int32_t n_q, double* d_quantiles, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- posterior predictive summaries: mean, variance and quantiles of the model output (extension) ----
 * The fitted curve with its uncertainty.  The reference's demos draw the model at the mean parameters as the "Est."
 * curve (demos/line_plus_noise/line_plus_noise.py:138,181), a plug-in estimate without a band; the summaries of
 * y_i = model(x_s; theta_i)[c] over the whole weighted cloud need n_settings x n_particles evaluations, which stay on
 * the chip here.  y_i is what obe_eval_over_particles writes for the setting x_s (obe_base.py:298-320), bit for bit;
 * d_settings (n_setdims, n_settings) with row stride ld_s holds POINTS, one per column.  NaN and negative weights
 * count as zero, and a particle of zero weight contributes nothing whatever its y is.  All results land in the
 * caller's DEVICE buffers, nothing is waited for.
 * d_ws: obe_predictive_workspace_bytes(n_particles, n_settings, the model's channels, n_q —
 * 0 for the moments —) bytes, a buffer of its own, as for the posterior summaries; the size does not shrink when an
 * argument grows. */
OBE_API int64_t obe_predictive_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_q);
/* d_mean, d_var (C, n_settings): mean = sum w y / sum w and var = sum w (y - mean)^2 / sum w, the weighted form of the
 * np.average / variance the reference takes of its parameters (particlepdf.py:173-214), in two passes over the
 * cloud (the second about the mean the first one found).  Partial sums are folded in a fixed order: the same bits
 * from run to run.  sum w == 0 gives NaN. */
OBE_API int obe_predictive_moments(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                           const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                           double* d_mean, double* d_var, void* d_ws, int64_t ws_bytes, void* stream);
/* d_quantiles (n_q, C, n_settings) = np.quantile(y, h_q, weights = w, method = "inverted_cdf") per setting and channel,
 * by obe_weighted_quantiles' rule and radix select (fixed-point weights, np.sort's order, the same bits under any
 * permutation of the cloud): the model values of up to 64 (setting, channel) rows at a time are written to the
 * workspace (64 x n_particles doubles of it) and selected from as from a cloud of rows.  1..16 values of q, each in
 * [0, 1]. */
OBE_API int obe_predictive_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                             const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                             const double* h_q, int32_t n_q, double* d_quantiles, void* d_ws, int64_t ws_bytes,
                             void* stream);

/* ---- posterior predictive of a MEASUREMENT: log-density and tail probabilities (extension) ----
 * Is a reading plausible under what the cloud has learnt?  The summaries above describe the model curve alone; a
 * reading carries its noise too: p(y | x, data) = sum_i w_i prod_c N(y_c; f_c(x; theta_i), sigma_c,i) / sum_i w_i, the
 * mixture whose terms the update multiplies the weights by (obe_base.py:269-271, :451-461; obe_noiseparam.py:109-120
 * with sigma from parameter rows) — without the choke, which tempers the update and is no density of y.  Taken for the
 * record about to be used it is the one-step model evidence.  A record is a column: the setting point d_settings
 * (n_setdims, n_records), the reading d_y_meas (C, n_records) — all C channels of the model — and its noise: exactly
 * one of d_sigma (C, n_records), known and free to differ per record, and h_noise_rows (C rows of the cloud).  With
 * f = what obe_eval_over_particles writes, bit for bit, and z_c = (f_c - y_c) / sigma_c:
 * a particle enters only with a weight > 0 (NaN and negative weights count as zero, whatever f is then) and with every
 * sigma of it > 0 (a NaN sigma fails; the update's nan_to_num zeroes such a particle's product).  n_records x
 * n_particles evaluations stay on the chip; partial results are folded in a fixed order: the same bits from run to
 * run.  All results land in the caller's DEVICE buffers, nothing is waited for.  d_ws:
 * obe_predictive_score_workspace_bytes(n_particles, n_records, the model's channels) bytes, a buffer of its own; the
 * size does not shrink when an argument grows. */
OBE_API int64_t obe_predictive_score_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels);
/* d_logpdf (n_records,) = log p(y | x, data), the joint density over the channels, as a running (max, scaled sum) pair
 * with one exp per evaluation: l_i = sum_c [-z_c^2 / 2 - log sigma_c], log p = m + log sum_i w_i exp(l_i - m) -
 * log sum w - (C / 2) log 2 pi.  A particle whose l_i is -inf or NaN contributes nothing; -inf if none contributed,
 * NaN if sum w == 0. */
OBE_API int obe_predictive_logpdf(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                          const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                          const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p,
                          int64_t n_particles, const double* d_weights, double* d_logpdf,
                          void* d_ws, int64_t ws_bytes, void* stream);
/* d_lower, d_upper (C, n_records) = P(Y_c <= y_c) and P(Y_c >= y_c) per channel: sum_i w_i erfc(z_c / sqrt 2) / 2 and
 * sum_i w_i erfc(-z_c / sqrt 2) / 2 over sum w.  Both are sums of positive terms (neither is 1 - the other), so a far
 * tail keeps its relative accuracy.  A NaN z contributes to neither; 0 if nothing contributed, NaN if sum w == 0. */
OBE_API int obe_predictive_tails(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                         const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                         const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p,
                         int64_t n_particles, const double* d_weights, double* d_lower, double* d_upper,
                         void* d_ws, int64_t ws_bytes, void* stream);

/* ---- posterior predictive of a measurement, inverted: quantiles of the NEXT READING (extension) ----
 * Where will the next reading fall?  The band to draw against measured points, an outlier threshold fixed before the
 * reading is taken, the range to set on an instrument: the inverse of obe_predictive_tails.  For a setting point x (a
 * column of d_settings), a channel c and a level q in (0, 1), with f = what obe_eval_over_particles writes, bit for bit:
 * a particle CONTRIBUTES to channel c with a weight > 0 (NaN and negative weights count as zero), every noise row of it
 * > 0 (h_noise_rows only) and a finite f_c — a stated deviation from the tails above, where +-inf counts as mass at
 * infinity: a reading cannot be infinite, and an infinite component would make the bracket infinite.  With T_c = sum w,
 * L_c(y) = sum w Phi((y - f_c) / sigma_c) and U_c(y) = sum w Phi((f_c - y) / sigma_c) over the contributing particles,
 * each a sum of positive terms formed as obe_predictive_tails forms them, the result is the y with L_c(y) = q T_c
 * (q <= 1/2) or U_c(y) = (1 - q) T_c (q > 1/2; 1 - q is exact there, so a far upper tail keeps its relative accuracy).
 * T_c == 0 (nobody contributes, sum w == 0 included) gives NaN.  The noise: exactly one of d_sigma (C, n_settings) with
 * row stride ld_sigma, known, finite and > 0 (a setting with another value gets NaN in every channel), and h_noise_rows
 * (C rows of the cloud).  The band is per channel, not joint; no choke.
 * h_q, h_z (n_q,), 1..16 levels: h_z[j] = the standard normal quantile of h_q[j], which the CALLER computes (finite; an
 * error of 1e-9 (1 + |z|) in it costs nothing but passes: it only places the first bracket).
 * Geometry of obe_predictive_tails (lane = setting, the particles of a chunk one after the other, setting tiles x
 * particle chunks, partials folded in chunk order, no atomics: the same bits from run to run).  One bracket pass over
 * the cloud (per level the min / max of f + (z -+ 1e-9 (1 + |z|)) sigma: a guaranteed bracket), then max_passes (1..64)
 * pairs of an iteration pass — at every open row's trial y the tail A and the density mass D = sum w phi(z) / sigma —
 * and a step kernel: Newton's method on log A, y -+ (A / D) log(A / target), safeguarded by the bracket (its midpoint
 * when the Newton point leaves the open bracket, is not finite, or the step exceeds half the previous one; a Newton
 * step below the resolution of y is taken as two ulp of y, so that the far end of the bracket comes in).  A row
 * closes when |A - target| <= 2^-36 target, or when its bracket is <= 4 ulp of its larger end (then at the midpoint).
 * Workgroups of a pass whose setting tile has no open row return at once; the whole budget is enqueued and NOTHING IS
 * WAITED FOR: d_quantiles (n_q, C, n_settings) and d_passes (n_q, C, n_settings; the passes a row used, >= 1; 0 for a
 * NaN row; -max_passes for a row still open at the end, which delivers its bracket's midpoint) land in the caller's
 * DEVICE buffers.  d_ws: obe_predictive_reading_workspace_bytes(n_particles, n_settings, the model's channels, n_q)
 * bytes, a buffer of its own; the size does not shrink when an argument grows. */
OBE_API int64_t obe_predictive_reading_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_q);
OBE_API int obe_predictive_reading_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                                     const double* d_sigma, int64_t ld_sigma, const int32_t* h_noise_rows,
                                     const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                                     const double* h_q, const double* h_z, int32_t n_q, int32_t max_passes,
                                     double* d_quantiles, int32_t* d_passes, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- design for parameters of interest: output-parameter covariance and the variance a reading removes (extension) ----
 * Every utility of the reference scores a setting by how much the model output varies there, for any reason
 * (obe_base.py:579-720: sum_c var_p / var_n); a user who wants ONE parameter and treats the others as nuisances needs
 * the covariance, over the weighted cloud, between the model output and that parameter.  With y_c,i = what
 * obe_eval_over_particles writes for the setting x, bit for bit, cleaned weights (NaN and negative weights count as
 * zero, a particle of zero weight contributes nothing whatever its y or theta is) and W = sum w:
 *   m_c(x)   = sum w y_c / W                               t_d = sum w theta_d / W
 *   S_cc'(x) = sum w (y_c - m_c)(y_c' - m_c') / W          V_d = sum w (theta_d - t_d)^2 / W
 *   K_dc(x)  = sum w (theta_d - t_d)(y_c - m_c) / W
 * in two passes over the cloud (the second about the means the first one found); n_settings x n_particles evaluations
 * stay on the chip.  Partial sums are folded in a fixed order: the same bits from run to run.  All results land in the
 * caller's DEVICE buffers, nothing is waited for.  h_rows: the n_rows parameter rows of interest (1..8 per call, each in
 * [0, n_dims), n_dims the rows of the cloud); d_ws: obe_output_covariance_workspace_bytes(n_particles, n_settings, the
 * model's channels, n_rows) bytes, a buffer of its own, as for the posterior predictive summaries. */
OBE_API int64_t obe_output_covariance_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels,
                                              int32_t n_rows);
/* d_mean (C, n_settings): obe_predictive_moments' mean, bit for bit (the same launches).  d_ycov (C (C + 1) / 2,
 * n_settings): the lower triangle of S, packed row-major (00, 10, 11, 20, ...); may be NULL (a later tile of rows of the
 * same request).  d_xcov (n_rows, C, n_settings): K.  d_pvar (n_rows,): V.  sum w == 0 gives NaN. */
OBE_API int obe_output_covariance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                          const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                          const double* d_weights, const int32_t* h_rows, int32_t n_rows, double* d_mean,
                          double* d_ycov, double* d_xcov, double* d_pvar, void* d_ws, int64_t ws_bytes,
                          void* stream);
/* d_gain (n_rows, n_settings): G_d(x) = k_d^T (S(x) + diag nu(x))^-1 k_d with k_d = K_d.(x) — the variance of theta_d
 * that the best LINEAR estimator of theta_d from one reading at x removes: exact for a model that is linear in its
 * parameters with a Gaussian cloud, in general a lower bound on the expected reduction Var(E[theta_d | y]).  By a
 * Cholesky factor L of S + diag nu (C <= 8, in registers, a lane per setting) and one forward solve per row, as the sum
 * of squares |L^-1 k_d|^2; a pivot that is not > 0 gives NaN for that setting.  d_ycov, d_xcov, d_pvar: what
 * obe_output_covariance left; d_noise_var: nu as (C,) with ld_noise == 0 or (C, n_settings) with row stride ld_noise.
 * d_utility (n_settings,): U(x) = [sum_d h_weights[d] G_d(x) / V_d] / cost(x), a term with V_d == 0 being 0; h_weights
 * NULL: 1 each; cost(x) = d_cost[x] if d_cost is given, else the scalar cost.  accumulate != 0: U is ADDED to what
 * d_utility holds (a later tile of rows of the same request); 0: it is stored.  d_gain and d_utility may each be NULL
 * (d_pvar is read for d_utility only).  n_rows 1..8, n_channels 1..OBE_MAX_CHANNELS.  Model-independent. */
OBE_API int obe_variance_reduction(const double* d_ycov, const double* d_xcov, int32_t n_rows, int32_t n_channels,
                           int64_t n_settings, const double* d_noise_var, int64_t ld_noise, const double* d_pvar,
                           const double* h_weights, const double* d_cost, double cost, double* d_gain,
                           double* d_utility, int32_t accumulate, void* stream);

/* ---- assimilating a recorded data set: joint log-likelihood of many records, tempered update (extension) ----
 * pdf_update() takes one reading at a time (obe_base.py:340-399); people with a recorded spectrum, yesterday's scan or
 * a second model to compare evidences loop it R times.  The same work as one computation is n_records x n_particles
 * model evaluations that stay on the chip: per particle the log of the product of the likelihoods the R updates would
 * multiply the weights by (obe_base.py:451-461; obe_noiseparam.py:109-120 with sigma from parameter rows) — without the
 * choke, which the caller applies as an exponent.  A record is a column, as for obe_predictive_logpdf: the setting point
 * d_settings (n_setdims, n_records), the reading d_y_meas (C, n_records) and its noise: exactly one of d_sigma
 * (C, n_records) and h_noise_rows (C rows of the cloud).  With f = what obe_eval_over_particles writes, bit for bit,
 * and z_rc = (f_c(x_r; theta_i) - y_rc) / sigma_rc:
 *   d_loglik[i] = sum_r sum_c [-z_rc^2 / 2 - log sigma_rc] - n_records (C / 2) log 2 pi
 * for EVERY particle, whatever its weight.  NaN marks "contributes nothing": a particle with a noise row that is not
 * > 0 (NaN included), a record with a sigma that is not > 0 (then every particle), a model output that is NaN or +-inf
 * (or a sum of z^2 that overflows).  accumulate != 0: the result is ADDED to what d_loglik holds (a later tile of
 * records of the same request, added in tile order); 0: it is stored.
 * Lane <-> particle, its rows in registers; the records are packed once per call into a table (setting, reading, 1 /
 * sigma) that is read with wave-uniform indices; sum log sigma is formed once per chunk of records (known sigma) or
 * once per particle (noise rows).  Per record and channel: z = (f - y) (1 / sigma), q = fma(z, z, q), in record order;
 * the chunk's term is -q / 2 - sum log sigma.  Grid = particle tiles x record chunks, the chunks' partial results are
 * added in chunk order: no atomics, the same bits from run to run.  Nothing is waited for.  d_ws:
 * obe_records_loglik_workspace_bytes(n_particles, n_records, the model's channels) bytes, a buffer of its own; the size
 * does not shrink when an argument grows. */
OBE_API int64_t obe_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels);
OBE_API int obe_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                       const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                       const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p, int64_t n_particles,
                       int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream);
/* The sums a tempered update chooses its step from: w'_i = w_i exp(a (l_i - m)) for up to OBE_TEMPERED_MAX_TRIALS
 * trial exponents a (each finite and >= 0) in one pass over the cloud (particlepdf.py:136-139 is w l / sum(w l), :236-258
 * tests 1 / sum(w'^2)).  NaN and negative weights count as zero; a particle whose l is not finite is skipped.
 *   h_sums[0] = m, the largest finite l over the particles whose weight is > 0 (-inf if there is none)
 *   h_sums[1] = sum w over those particles
 *   h_sums[2 + 2 t], h_sums[3 + 2 t] = S1 = sum w exp(a_t (l - m)), S2 = sum (w exp(a_t (l - m)))^2
 * so that N_eff at exponent a_t is S1^2 / S2 and the evidence of the step log(S1 / sum w) + a_t m.  Block partials are
 * folded in a fixed order, as obe_weight_sums folds its own.  (sync): the 2 + 2 n_trials words reach the host as
 * obe_weight_sums' two do (h_sums page-locked: written by the last kernel and watched; else copied).  d_ws: at least
 * OBE_TEMPERED_WS_BYTES bytes.  Model-independent.  (h_sums is obe_weight_sums' h_out: the delivery audit keeps the
 * rule of this call in a table of its own, _audit._BATCH_RULES, and reads the arguments by these names.) */
#define OBE_TEMPERED_MAX_TRIALS 16
#define OBE_TEMPERED_WS_BYTES 131072
OBE_API int obe_tempered_sums(const double* d_loglik, const double* d_weights, int64_t n_particles,
                      const double* h_exponents, int32_t n_trials, void* d_ws, int64_t ws_bytes, double* h_sums,
                      void* stream);
/* d_lik_out[i] = exp(exponent (d_loglik[i] - shift)), and 0 where d_loglik[i] is not finite (NaN: nan_to_num's 0 of
 * particlepdf.py:136-139; +inf as well — a stated deviation: nan_to_num would make it 1.8e308).  What
 * obe_bayes_update_lik then multiplies the weights by.  No sync.  Model-independent. */
OBE_API int obe_tempered_likelihood(const double* d_loglik, int64_t n_particles, double exponent, double shift,
                            double* d_lik_out, void* stream);

/* ---- design of a batch of measurements: output-output covariance and greedy conditioning (extension) ----
 * opt_setting() answers "which ONE setting next"; an instrument that takes several points per round trip needs n
 * settings that are jointly informative: the second must account for what the first will already have taught.  The
 * quantity that needs is the covariance, over the weighted cloud, between the model output at every setting x and the
 * output at an already chosen "pivot" point p.  With y, the cleaned weights, W and m_c(x) as for obe_output_covariance:
 *   X_c'c(p, x) = sum w (y_c'(p) - m_c'(p)) (y_c(x) - m_c(x)) / W                     (X(x, x) is S(x))
 * d_pivots (n_setdims, n_pivots) with row stride ld_pivots; n_pivots x C <= 8 rows per call.  d_mean (C, n_settings):
 * mean_given != 0: an input, what obe_predictive_moments left for these settings; 0: computed here by the same launches
 * (the same bits) and left there.  The pivots' means are formed inside the call, as a request of their own.
 * d_cross (n_pivots, C, C, n_settings): [j, c', c, s] = X_c'c(p_j, x_s).  A table u_r,i = w_i (y_r(p; theta_i) - m_r) of
 * the rows is written once per call (lane <-> particle; a particle of zero weight is never evaluated); the pass has
 * obe_output_covariance's geometry and per evaluation the exact model, C subtractions and rows x C FMAs.  Chunk partials
 * are folded in chunk order: no atomics, the same bits from run to run, for the pivots in any order and for any prefix
 * of them.  sum w == 0 gives NaN.  Nothing is waited for.  d_ws: obe_output_cross_covariance_workspace_bytes(n_particles,
 * n_settings, the model's channels, n_pivots) bytes, a buffer of its own; the size does not shrink when an argument
 * grows. */
OBE_API int64_t obe_output_cross_covariance_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels,
                                                    int32_t n_pivots);
OBE_API int obe_output_cross_covariance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                                const double* d_pivots, int64_t ld_pivots, int32_t n_pivots,
                                const double* d_particles, int64_t ld_p, int64_t n_particles,
                                const double* d_weights, double* d_mean, int32_t mean_given, double* d_cross,
                                void* d_ws, int64_t ws_bytes, void* stream);
/* One step of the greedy design under the linear-Gaussian reading of obe_variance_reduction: conditions the output
 * variance of every setting on one more planned reading, at the setting pivot_index, and scores what is left.  A
 * reading is C scalar readings with noise nu_c'(p), taken in channel order; row m = rows_done + c':
 *   a(c, x)   = X_c'c(p, x) - sum_{m' < m} L_m'(c, x) L_m'(c', p)         g = a(c', p) + nu_c'(p)
 *   L_m(c, x) = a(c, x) / sqrt(g)        v_c(x) -= L_m(c, x)^2            *d_info += log(g / nu_c'(p)) / 2
 *   U(x)      = [sum_c v_c(x) / nu_c(x)] / cost(x)
 * d_cross (C, C, n_settings): the pivot's block of obe_output_cross_covariance; NULL: nothing is conditioned on, U is
 * formed from d_cvar as it is (with d_cvar = the variance of obe_predictive_moments: the variance utility).  d_factors
 * (max_rows, C, n_settings): rows [0, rows_done) are read, rows [rows_done, rows_done + C) written.  d_cvar (C,
 * n_settings): v, in and out.  d_noise_var, ld_noise, d_cost, cost: as for obe_variance_reduction.  d_taken (n_settings,)
 * bytes or NULL: a setting with a non-zero entry is never chosen.  d_utility (n_settings,): U.  d_best: 16 bytes, the
 * largest FINITE utility (a double) and the first index that has it (an int64) — a NaN or infinite utility is never
 * chosen, unlike np.argmax; NaN and -1 if there is none.  A g that is not > 0 or not finite makes its row NaN, and with
 * it everything that follows.  Every thread forms the pivot column's values itself: nothing written by a launch is read
 * by that launch.  After all rows *d_info = log det(I + N^-1/2 K_AA N^-1/2) / 2 in nats.  Exact for a model that is
 * linear in its parameters with a Gaussian cloud, an approximation otherwise.  Everything stays in DEVICE memory, nothing
 * is waited for.  Model-independent. */
OBE_API int obe_design_step(const double* d_cross, int64_t pivot_index, double* d_factors, int32_t rows_done,
                    int32_t max_rows, double* d_cvar, int32_t n_channels, int64_t n_settings,
                    const double* d_noise_var, int64_t ld_noise, const double* d_cost, double cost,
                    const uint8_t* d_taken, double* d_utility, double* d_best, double* d_info, void* stream);
/* One step of the greedy design FOR PARAMETERS OF INTEREST: obe_design_step's conditioning applied to the blocks of
 * obe_output_covariance — the whole S(x) (C x C) and K_dc(x) = cov(theta_d, y_c(x)) — and obe_variance_reduction's score
 * of what is left.  With a, g and L_m as for obe_design_step (row m = rows_done + c', the rows of earlier calls read
 * from d_factors):
 *   b(d)      = K_dc'(p) - sum_{m' < m} T_m'(d) L_m'(c', p)           T_m(d) = b(d) / sqrt(g)
 *   S_cc''(x) -= L_m(c, x) L_m(c'', x)      K_dc(x) -= T_m(d) L_m(c, x)      Vleft_d -= T_m(d)^2
 *   G_d(x)    = k_d(x)^T (S(x) + diag nu(x))^-1 k_d(x)                U(x) = [sum_d h_weights[d] G_d(x) / V_d] / cost(x)
 * d_cross (C, C, n_settings): the pivot's block of obe_output_cross_covariance; NULL: nothing is conditioned on, the
 * score is formed from d_ycov and d_xcov as they are (with what obe_output_covariance left: obe_variance_reduction's
 * d_gain and d_utility, bit for bit — the same kernel in the same tiles of 8 rows).  d_factors (max_rows, C, n_settings)
 * and d_tstore (max_rows, n_sel): rows [0, rows_done) are read (d_factors), rows [rows_done, rows_done + C) written,
 * nothing beyond.  d_ycov (C (C + 1) / 2, n_settings), packed as obe_output_covariance packs it, and d_xcov (n_sel, C,
 * n_settings): in and out.  d_pvar (n_sel,): V, the UNCONDITIONED variance of the rows of interest, read only (a term
 * with V_d == 0 is 0).  d_pvar_left (n_sel,): Vleft, in and out (the caller starts it at V); after the rows of the picks A
 * it is V_d - k_A^T (K_AA + N_A)^-1 k_A, and what the C rows of a pick remove of it is the G_d that chose the pick.
 * h_weights (n_sel,) or NULL (1 each): an input, read before the call returns.  d_noise_var, ld_noise, d_cost, cost,
 * d_taken, d_best: as for obe_design_step.  d_gain (n_sel, n_settings) and d_utility (n_settings,) are both written.
 * n_sel 1..OBE_MAX_DIMS, n_channels 1..OBE_MAX_CHANNELS.  T_m needs K at the pivot's column, which the grid-wide launch
 * rewrites: a launch of one workgroup forms the T rows of the pick first and the grid-wide launch reads them — nothing
 * written by a launch is read by another thread of that launch.  A g that is not > 0 or not finite makes its rows NaN,
 * and with them everything that follows.  Exact for a model that is linear in its parameters with a Gaussian cloud, a
 * heuristic otherwise, and greedy.  Everything stays in DEVICE memory, nothing is waited for.  Model-independent. */
OBE_API int obe_design_interest_step(const double* d_cross, int64_t pivot_index, double* d_factors, double* d_tstore,
                             int32_t rows_done, int32_t max_rows, double* d_ycov, double* d_xcov, int32_t n_sel,
                             int32_t n_channels, int64_t n_settings, const double* d_noise_var, int64_t ld_noise,
                             const double* d_pvar, double* d_pvar_left, const double* h_weights, const double* d_cost,
                             double cost, const uint8_t* d_taken, double* d_gain, double* d_utility, double* d_best,
                             void* stream);

/* ---- measurement noise that depends on the signal (extension) ----
 * Every other call takes the noise of a reading as a number per channel or as a parameter row.  The reference names the
 * case neither covers and leaves it out (obe_base.py:542-564: noise that "depends on the measurement value, like
 * root(N), Poisson-like counting noise" needs the noise model averaged over the distribution).  Here the noise variance
 * of a reading whose noise-free value is y is, per channel c of the model,
 *   nu_c(y) = a_c + b_c |y| + c_c y^2
 * h_noise_coef: 3 doubles per channel of the model, {a, b, c} channel after channel; each finite and >= 0, and in every
 * channel one of them > 0 (else -1 before any launch).  y_c,i = what obe_eval_over_particles writes, bit for bit.  All
 * results land in the caller's DEVICE buffers, nothing is waited for.
 * d_lik (n_particles,): what obe_bayes_update_lik multiplies the weights by,
 *   L_i = prod_{c < n_lik_channels} exp(-(y_c,i - h_y_meas[c])^2 / (2 nu_c(y_c,i))) / sqrt(nu_c(y_c,i))
 * (obe_base.py:418-461 with sigma^2 = nu: no 1 / sqrt(2 pi), channels truncated as :453-455), as one exp of the summed
 * exponent over one product of square roots, then L^choke unless choke is NaN.  A particle with a nu_c that is not > 0
 * or not finite gets L = 0.  d_y == NULL: the model is evaluated at h_setting (n_setdims values; NULL: zeros) on the
 * cloud d_particles; d_y given, (C, n_particles) rows ld_y apart with C the model's channels: those values are used and
 * neither d_particles nor h_setting is read.  Both forms give the same bits.  Lane <-> particle, one stream over the
 * cloud. */
OBE_API int obe_signal_noise_likelihood(const obe_model* m, const double* d_y, int64_t ld_y,
                                const double* d_particles, int64_t ld_p, int64_t n_particles, const double* h_setting,
                                const double* h_y_meas, const double* h_noise_coef, int32_t n_lik_channels, double choke,
                                double* d_lik, void* stream);
/* d_noise_var (C, n_settings) = nu_bar_c(x_s) = a_c + b_c sum w |y_c| / W + c_c sum w y_c^2 / W over the whole weighted
 * cloud, W = sum w: the noise variance a sweep divides by (obe_sweep_utility's d_noise_var with noise_ld = n_settings).
 * NaN and negative weights count as zero, a particle of zero weight contributes nothing whatever its y is, W == 0 gives
 * NaN.  d_settings (n_setdims, n_settings) with row stride ld_s: a slice of a grid is its first column's address with
 * the grid's stride.  obe_predictive_moments' geometry (lane = setting, the particles of a chunk one after the other,
 * setting tiles x particle chunks) in ONE pass: both sums are of non-negative terms and need no centring, and W rides
 * along.  Chunk partials are folded in chunk order: no atomics, the same bits from run to run — and for a slice the bits
 * of those columns of the whole grid's call while the cloud decides the number of chunks (n_particles <= 256 x 8192 /
 * the grid's tiles of 64 settings).  d_ws: obe_signal_noise_workspace_bytes(n_particles, n_settings, the model's
 * channels) bytes, a buffer of its own; the size does not shrink when an argument grows. */
OBE_API int64_t obe_signal_noise_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels);
OBE_API int obe_signal_noise_variance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                              const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                              const double* h_noise_coef, double* d_noise_var, void* d_ws, int64_t ws_bytes,
                              void* stream);
/* K19 — assimilating a recorded data set with THIS likelihood (extends obe_records_loglik, above, and the likelihood
 * of this section): per particle the log of the product of the factors obe_signal_noise_likelihood gives for the records,
 * with the 1 / sqrt(2 pi) it leaves out, and without the choke.  A record is a column, as obe_records_loglik takes
 * records: the setting point d_settings (n_setdims, n_records) and the reading d_y_meas (C, n_records) of ALL C channels
 * of the model.  With f = what obe_eval_over_particles writes, bit for bit, and nu = a_c + b_c |f| + c_c f^2 (the
 * arithmetic of the likelihood's nu):
 *   d_loglik[i] = sum_r sum_c [-(f_c(x_r; theta_i) - y_rc)^2 / (2 nu) - log(nu) / 2] + constant
 * for EVERY particle, whatever its weight.  constant: a finite host double, the particle-independent part of the call's
 * records (-n_records C log(2 pi) / 2 makes d_loglik the full log density).  NaN where any nu of the particle is not
 * > 0 or not finite: a NaN or +-inf model output lands here, and so does a NaN reading.  h_noise_coef: as above.
 * accumulate != 0: the result is ADDED to what d_loglik holds (a later tile of records of the same request, added in
 * tile order); 0: it is stored.  obe_records_loglik's geometry: lane <-> particle, its rows in registers; the records
 * are packed once per call into a table (setting | y) that is read with wave-uniform indices; grid = particle tiles x
 * record chunks of at least 32 records, the chunk partials added in chunk order: no atomics, the same bits from run to
 * run, and a permuted cloud gives the permuted bits.  Per evaluation and channel one division and one log.  Nothing is
 * waited for.  d_ws: obe_signal_noise_records_loglik_workspace_bytes(n_particles, n_records, the model's channels)
 * bytes, a buffer of its own; the size does not shrink when an argument grows. */
OBE_API int64_t obe_signal_noise_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels);
OBE_API int obe_signal_noise_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                                    const double* d_y_meas, int64_t ld_y, const double* h_noise_coef, double constant,
                                    const double* d_particles, int64_t ld_p, int64_t n_particles, int32_t accumulate,
                                    double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream);
/* K21 — the posterior predictive of a READING under THIS noise: obe_predictive_logpdf, obe_predictive_tails and
 * obe_predictive_reading_quantiles (above) with h_noise_coef in place of their d_sigma, ld_sigma, h_noise_rows.  The
 * predictive is still a mixture of n_particles Gaussians; component i of channel c has the mean f_c(x; theta_i) — what
 * obe_eval_over_particles writes, bit for bit — and the variance nu_c(f_c(x; theta_i)) = a_c + b_c |f| + c_c f^2, the
 * arithmetic of the likelihood's nu (an f whose square overflows behaves as it does there).  Who CONTRIBUTES is the
 * likelihood's rule: a particle with a weight > 0 (NaN and negative weights count as zero) whose nu is > 0 and finite in
 * EVERY channel.  A NaN or +-inf model value in ANY channel therefore removes the particle from ALL channels — a stated
 * difference from obe_predictive_tails, where +-inf counts as mass at infinity.  The normalisers are those of the calls
 * above: the density and the tails divide by the sum of ALL positive weights (a left-out particle is counted there: its
 * likelihood is 0, which keeps the density the one-step evidence); the quantiles use T = sum w over the contributing
 * particles, the same for every channel.  h_noise_coef: as above, -1 before any launch.  The geometry of the calls above:
 * lane = record or setting, the particles of a chunk one after the other, setting tiles x particle chunks (x level
 * groups), chunk partials folded in chunk order, no atomics: the same bits from run to run.  All results land in the
 * caller's DEVICE buffers, nothing is waited for.
 * d_logpdf (n_records,) = log(sum_i w_i prod_c N(y_c; f_c,i, nu_c,i) / sum w) as a running (max, scaled sum) pair,
 * l_i = sum_c [-(f_c - y_c)^2 / (2 nu_c) - log(nu_c) / 2] (obe_signal_noise_records_loglik's term for one record), minus
 * (C / 2) log 2 pi; -inf if nobody contributed, NaN if sum w == 0.
 * d_lower, d_upper (C, n_records) = sum w erfc(+-z_c / sqrt 2) / 2 over sum w with z_c = (f_c - y_c) / sqrt(nu_c), both
 * sums of positive terms; 0 if nobody contributed, NaN if sum w == 0.  d_ws of both:
 * obe_predictive_score_workspace_bytes(n_particles, n_records, the model's channels) bytes, a buffer of its own.
 * d_quantiles, d_passes (n_q, C, n_settings): obe_predictive_reading_quantiles' levels (h_q, h_z, 1..16 of them), bracket
 * (per level the min of f + z_lo sqrt(nu) and the max of f + z_hi sqrt(nu): it holds for a width per particle), pass
 * budget (max_passes 1..64), Newton step on log A, stopping rule and pass counts; D = sum w phi(z) / sqrt(nu), sqrt(nu)
 * and its reciprocal formed once per (setting, particle, channel) and shared by a level group.  T == 0 gives NaN.  d_ws:
 * obe_predictive_reading_workspace_bytes(n_particles, n_settings, the model's channels, n_q) bytes, a buffer of its
 * own. */
OBE_API int obe_signal_noise_logpdf(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                            const double* d_y_meas, int64_t ld_y, const double* h_noise_coef,
                            const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                            double* d_logpdf, void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_signal_noise_tails(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                           const double* d_y_meas, int64_t ld_y, const double* h_noise_coef,
                           const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                           double* d_lower, double* d_upper, void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_signal_noise_reading_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s,
                                       int64_t n_settings, const double* h_noise_coef, const double* d_particles,
                                       int64_t ld_p, int64_t n_particles, const double* d_weights, const double* h_q,
                                       const double* h_z, int32_t n_q, int32_t max_passes, double* d_quantiles,
                                       int32_t* d_passes, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- yes/no outcomes: binomial likelihood and information-gain design (extension) ----
 * Every likelihood above is Gaussian.  Here the model's channel c gives a success probability p_c = f_c(x; theta) and a
 * record holds k_c successes in n_c shots per channel (a click or no click; k clicks in n shots).  Models of at most
 * OBE_BINOMIAL_MAX_CHANNELS channels (else -1 before any launch).  p_c,i = what obe_eval_over_particles writes, bit for
 * bit.  All results land in the caller's DEVICE buffers, nothing is waited for.
 * d_lik (n_particles,): what obe_bayes_update_lik multiplies the weights by,
 *   L_i = exp(sum_{c < n_lik_channels} [k_c log p_c,i + (n_c - k_c) log1p(-p_c,i)])
 * with k_c = h_successes[c], n_c = h_shots[c] (n_lik_channels values each: finite, integer-valued, 0 <= k_c <= n_c,
 * n_c >= 1, else -1), a term whose count is 0 skipped (p = 0 with k = 0 contributes the factor 1), then L^choke unless
 * choke is NaN.  No binomial coefficient: it is the same for every particle.  A particle with any p_c — of all the
 * model's channels — that is NaN or outside [0, 1] gets L = 0.  d_y, d_particles, h_setting: as
 * obe_signal_noise_likelihood takes them, but h_setting == NULL with d_y == NULL is -1 here (no setting to evaluate the
 * model at); both forms give the same bits.  Lane <-> particle, one stream over the cloud. */
#define OBE_BINOMIAL_MAX_CHANNELS 3
OBE_API int obe_binomial_likelihood(const obe_model* m, const double* d_y, int64_t ld_y, const double* d_particles,
                            int64_t ld_p, int64_t n_particles, const double* h_setting, const double* h_successes,
                            const double* h_shots, int32_t n_lik_channels, double choke, double* d_lik, void* stream);
/* d_information (n_settings,): the exact mutual information, in nats, between theta and the joint outcome
 * o in {0 .. 2^C - 1} of ONE shot in every channel (independent given theta, not marginally: enumerated), per unit cost,
 *   Pbar_o = sum_i w_i prod_c (bit c of o ? p_c,i : 1 - p_c,i) / W
 *   hbar   = sum_i w_i sum_c h2(p_c,i) / W,   h2(p) = -p log p - (1 - p) log1p(-p),  0 log 0 = 0
 *   U      = max(-sum_o Pbar_o log Pbar_o - hbar, 0) / cost       (the clamp covers rounding; NaN stays NaN)
 * d_noise_var (C, n_settings) = sum_i w_i p_c,i (1 - p_c,i) / W / shots: the variance of the fraction k / n of `shots`
 * (finite, >= 1) shots, the noise variance a Gaussian utility divides by (obe_sweep_utility's d_noise_var with
 * noise_ld = n_settings).  Either output may be NULL, not both; what is written has the same bits whichever other output
 * is asked for.  W sums the contributing particles only: NaN and negative weights count as zero, a particle of zero
 * weight contributes nothing whatever its p is, and neither does, at a setting, a particle with a p_c there that is NaN or
 * outside [0, 1]; W == 0 gives NaN.  cost = cost if d_cost == NULL else d_cost[s] (obe_utility_argmax's convention).
 * d_settings, the geometry, the chunk partials folded in chunk order (no atomics: the same bits from run to run, and for
 * a slice the bits of those columns of the whole grid's call while the cloud decides the number of chunks) and d_ws:
 * as obe_signal_noise_variance, with 2^C + C + 2 sums per lane and obe_binomial_workspace_bytes(n_particles, n_settings,
 * the model's channels) bytes; the size does not depend on n_particles and does not shrink when an argument grows. */
OBE_API int64_t obe_binomial_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels);
OBE_API int obe_binomial_information(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                             const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                             double shots, const double* d_cost, double cost, double* d_information,
                             double* d_noise_var, void* d_ws, int64_t ws_bytes, void* stream);
/* K19 — assimilating a recorded data set with THIS likelihood (extends obe_records_loglik and
 * obe_binomial_likelihood): a record is a column — the setting point d_settings (n_setdims, n_records), the successes
 * d_successes (C, n_records) and the shots d_shots (C, n_records) of ALL C channels of the model.  With p = what
 * obe_eval_over_particles writes, bit for bit:
 *   d_loglik[i] = sum_r sum_c [k_rc log p_c(x_r; theta_i) + (n_rc - k_rc) log1p(-p_c(x_r; theta_i))] + constant
 * for EVERY particle, whatever its weight; a term whose count is 0 is skipped (p = 0 with k = 0 contributes nothing).
 * constant: a finite host double (sum_r sum_c log C(n_rc, k_rc) makes d_loglik the full log density).  NaN where any
 * p_c of the particle at any record is NaN or outside [0, 1]; otherwise -inf where p = 0 meets k > 0 or p = 1 meets
 * n - k > 0.  A record whose data cannot be one — k or n not finite or not whole, k < 0, n < 1, k > n — makes its chunk
 * of records, and with it d_loglik, NaN for every particle (obe_records_loglik's rule for a sigma that is not > 0).
 * Models of at most OBE_BINOMIAL_MAX_CHANNELS channels, else -1 before any launch.  accumulate, the geometry (the table
 * holds setting | k | n - k, the difference formed once per record), the chunk partials folded in chunk order (no
 * atomics: the same bits from run to run, a permuted cloud gives the permuted bits) and d_ws: as
 * obe_signal_noise_records_loglik, with obe_binomial_records_loglik_workspace_bytes.  Per evaluation and channel one
 * log and one log1p.  Nothing is waited for. */
OBE_API int64_t obe_binomial_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels);
OBE_API int obe_binomial_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                                const double* d_successes, int64_t ld_k, const double* d_shots, int64_t ld_n,
                                double constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                                int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- counted events: Poisson likelihood and exact information design (extension) ----
 * The model's channel c gives a RATE r_c = f_c(x; theta) in counts per unit exposure; a record holds k_c counted events
 * (whole numbers >= 0) in the exposure t_c (finite, > 0) per channel, lambda_c,i = t_c r_c,i.  r_c,i = what
 * obe_eval_over_particles writes, bit for bit.  All results land in the caller's DEVICE buffers, nothing is waited for.
 * d_lik (n_particles,): what obe_bayes_update_lik multiplies the weights by,
 *   L_i = exp(sum_{c < n_lik_channels} [k_c log lambda_c,i - lambda_c,i - log k_c!])
 * with k_c = h_counts[c], t_c = h_exposure[c], log k_c! = h_logfact[c] (the host's lgamma(k_c + 1); n_lik_channels values
 * each, n_lik_channels in 0..the model's channels; a count that is not a whole number >= 0 or an exposure that is not
 * finite and > 0 is -1), then L^choke unless choke is NaN.  log k! is kept although it is the same for every particle:
 * every exponent is then <= 0 and L is the Poisson pmf itself (k = lambda = 1000 would otherwise ask for exp(5908)).  A
 * channel with k_c = 0 contributes -lambda alone, no log: lambda = 0 with k = 0 is the factor 1, lambda = 0 with k > 0
 * gives L = 0.  A particle with any r_c — of all the model's channels — that is NaN, negative or +inf (or whose t_c r_c
 * overflows) gets L = 0.  d_y, d_particles, h_setting: as obe_binomial_likelihood takes them; both forms give the same
 * bits.  Lane <-> particle, one stream over the cloud.
 *
 * obe_poisson_information, models of ONE channel: the exact mutual information, in nats, between theta and the next
 * reading's count CENSORED at cap, outcomes {0, 1, .., cap - 1, ">= cap"}, per unit cost.  With lambda_i = exposure r_i,
 *   p_k,i  = Pois(k; lambda_i) for k < cap,   tau_i = max(1 - sum_{k < cap} p_k,i, 0)
 *   Pbar_k = sum_i w_i p_k,i / W,             taubar = sum_i w_i tau_i / W
 *   h_i    = -sum_{k < cap} p_k,i (k log lambda_i - lambda_i - log k!) - tau_i log tau_i
 *            (log lambda reads as 0 at lambda = 0; 0 log 0 = 0)
 *   U      = max(-sum_k Pbar_k log Pbar_k - taubar log taubar - sum_i w_i h_i / W, 0) / cost
 * (the clamp covers rounding; NaN stays NaN).  Exact for the censored reading; by data processing a lower bound of the
 * uncensored reading's information, tight when taubar is small: taubar is an output, so that a cap too small for the
 * rates shows.  cap is 16, 32 or 64 (OBE_POISSON_MAX_CAP; compile-time sizes: the outcome sums stay in registers), else
 * -1.  The kernel forms p_0 = exp(-lambda), p_k = p_k-1 (lambda (1 / k)) and, since k p_k = lambda p_k-1, the sum in h_i
 * as log lambda . lambda sum_{k < cap - 1} p_k - lambda sum_k p_k - sum_k p_k log k!: one exp and two log per evaluation.
 * (Beyond lambda ~ 708, where exp(-lambda) is subnormal, the p_k — all below 1e-200 — lose relative accuracy; tau = 1.)
 *   d_information (n_settings,) = U;  d_tail (n_settings,) = taubar;
 *   d_pmf (cap + 1, n_settings): the rows Pbar_0 .. Pbar_cap-1, then taubar — the predicted histogram of the next reading;
 *   d_noise_var (C, n_settings) = sum_i w_i r_c,i / W / exposure: the variance of the reading k / t in the model's units,
 *     the noise variance a Gaussian utility divides by (obe_sweep_utility's d_noise_var with noise_ld = n_settings).
 * Any output may be NULL, not all of them; what is written has the same bits whichever other outputs are asked for.
 * d_information, d_tail or d_pmf with a model of more than one channel is -1; d_noise_var alone works for every channel
 * count (an instantiation that carries no outcome sums).  W sums the contributing particles only: NaN and negative
 * weights count as zero, a particle of zero weight contributes nothing whatever its rate is, and neither does, at a
 * setting, a particle with an r_c there that is not a rate (NaN, negative, +inf, or exposure r_c overflows); W == 0 gives
 * NaN.  cost = cost if d_cost == NULL else d_cost[s] (obe_utility_argmax's convention).  d_settings, the geometry, the
 * chunk partials folded in chunk order (no atomics: the same bits from run to run, and for a slice the bits of those
 * columns of the whole grid's call while the cloud decides the number of chunks) and d_ws: as obe_binomial_information,
 * with cap + C + 3 sums per lane and obe_poisson_workspace_bytes(n_particles, n_settings, the model's channels, cap)
 * bytes; the size does not depend on n_particles and does not shrink when an argument grows. */
#define OBE_POISSON_MAX_CAP 64
OBE_API int obe_poisson_likelihood(const obe_model* m, const double* d_y, int64_t ld_y, const double* d_particles,
                           int64_t ld_p, int64_t n_particles, const double* h_setting, const double* h_counts,
                           const double* h_exposure, const double* h_logfact, int32_t n_lik_channels, double choke,
                           double* d_lik, void* stream);
OBE_API int64_t obe_poisson_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t cap);
OBE_API int obe_poisson_information(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                            const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                            double exposure, int32_t cap, const double* d_cost, double cost, double* d_information,
                            double* d_tail, double* d_pmf, double* d_noise_var, void* d_ws, int64_t ws_bytes,
                            void* stream);
/* K19 — assimilating a recorded data set with THIS likelihood (extends obe_records_loglik and obe_poisson_likelihood):
 * a record is a column — the setting point d_settings (n_setdims, n_records), the counted events d_counts
 * (C, n_records) and the exposures d_exposure (C, n_records) of ALL C channels of the model.  With r = what
 * obe_eval_over_particles writes, bit for bit, and lambda = t_rc r_c(x_r; theta_i):
 *   d_loglik[i] = sum_r sum_c [k_rc log lambda - lambda] + constant
 * for EVERY particle, whatever its weight; a channel with k = 0 contributes -lambda alone.  constant: a finite host
 * double (-sum_r sum_c log k_rc! makes d_loglik the full log density).  NaN where any r_c of the particle at any record
 * is not a rate (NaN, negative, +inf, or t r overflows); otherwise -inf where lambda = 0 meets k > 0.  A record whose
 * data cannot be one — k not a whole number >= 0, t not finite and > 0 — makes its chunk of records, and with it
 * d_loglik, NaN for every particle.  accumulate, the geometry (the table holds setting | k | t), the chunk partials
 * folded in chunk order (no atomics: the same bits from run to run, a permuted cloud gives the permuted bits) and d_ws:
 * as obe_signal_noise_records_loglik, with obe_poisson_records_loglik_workspace_bytes.  Per evaluation and channel one
 * log.  Nothing is waited for. */
OBE_API int64_t obe_poisson_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels);
OBE_API int obe_poisson_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                               const double* d_counts, int64_t ld_k, const double* d_exposure, int64_t ld_t,
                               double constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                               int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- K20 — count-aware scoring and reading bands (extension; no reference counterpart: extends K17/K18/K19) ----
 * "Is this count plausible?" and "where will the next count fall?" for the two counting likelihoods above.  law is
 * OBE_COUNT_BINOMIAL (the model's channel c gives p_c, a point's side datum is its shots n_c: whole, 1 ..
 * OBE_COUNT_MAX_OUTCOMES) or OBE_COUNT_POISSON (r_c, the exposure t_c: finite, > 0), anything else -1.  A POINT is a
 * column — the setting d_settings (n_setdims, n_points) and the side data d_side (C, n_points), rows ld_side apart —: a
 * setting of a design grid, or the setting of a record with its own n or t.  P_c,i(k) = Binomial(k; n_c, p_c,i) or
 * Poisson(k; t_c r_c,i), with p and r what obe_eval_over_particles writes, bit for bit.  At a point a particle
 * contributes when its weight is > 0 (NaN and negative weights count as zero) and EVERY channel's value there is one the
 * law takes (p in [0, 1]; r >= 0 with t r finite); W sums the contributing weights, W == 0 — also a point whose side
 * data are not valid — gives NaN.  All results land in the caller's DEVICE buffers, nothing is waited for.
 *
 * obe_count_table: d_pmf (C, count_max + 2, n_points) = Pbar_c(k) = sum_i w_i P_c,i(k) / W for k = 0 .. count_max, then
 * the mass above count_max, max(1 - sum_k Pbar_c(k), 0) — formed from the rows (a difference of numbers near 1: absolute
 * accuracy, about the rows' own N_p eps at worst), and exactly 0 for a binomial point with n_c <= count_max.  count_max
 * in 0 .. OBE_COUNT_MAX_OUTCOMES, else -1.  d_logfact (OBE_COUNT_MAX_OUTCOMES + 2,): log k! for k = 0 ..
 * OBE_COUNT_MAX_OUTCOMES + 1 on the device, the host's lgamma(k + 1) (obe_poisson_likelihood's h_logfact, as a table).
 * Geometry: obe_poisson_information's (one wave per workgroup, lane <-> point, particle chunks streamed, chunk partials
 * folded in chunk order: no atomics, the same bits from run to run), the outcomes in blocks of 32 (count_max < 32) or 64
 * outcome sums per lane, one launch per channel and block, each folded into its rows before the next starts.  Every
 * block starts from a log-space value of one of its own outcomes, so that the table is right where e^-lambda, (1 - p)^n
 * or p^n underflows (rows below ~1e-290 lose relative accuracy, as everywhere) and a recurrence's error grows over one
 * block only.  Poisson: exp(k0 log lambda - lambda - log k0!) of the block's first outcome k0, then
 * P(k) = P(k - 1) lambda / k.  Binomial: a lane sums Cmax p^k (1 - p)^(n - k), Cmax the block's largest C(n, k), a
 * geometric sequence in k that is run from its large end — upwards from k0 for p <= 1/2, downwards from the block's last
 * outcome <= n for p > 1/2 — and the fold multiplies by C(n, k) / Cmax: right wherever in the block the mass lies
 * (p = 1e-12 and p = 1 - 1e-12 alike).  lambda = 0, p = 0 and p = 1 give the exact point masses.  With one channel,
 * exposure the same for all points and count_max = cap - 1 the Poisson rows k < cap hold the bits of
 * obe_poisson_information's d_pmf (the same arithmetic in the same order; tests/test_gpu_counts.py asserts it).  d_ws:
 * obe_count_workspace_bytes(n_particles, n_points, the model's channels, count_max) bytes; the size depends on n_points
 * alone (not on count_max: a block's partials are K18's size) and does not shrink when an argument grows.
 *
 * obe_count_tails, obe_count_quantiles: light kernels on a table obe_count_table wrote, one thread per (point, channel);
 * they take no model.  d_counts (C, n_points), rows ld_k apart: d_lower = sum_{j <= k} Pbar_c(j), d_upper = sum_{j >= k}
 * Pbar_c(j) + the mass above, both (C, n_points), each summed from its small end; both include k itself; either may be
 * NULL, not both; NaN where k is not a whole number in 0 .. count_max.  h_levels: n_levels (1 .. OBE_COUNT_MAX_LEVELS)
 * host doubles in the open interval (0, 1), else -1; d_quantiles (n_levels, C, n_points) = the smallest k with
 * sum_{j <= k} Pbar_c(j) >= q (where the mass above is exactly 0 the last row closes the sum: 1), +inf where count_max
 * is too small for the level, NaN where W == 0.
 *
 * obe_count_logpmf: d_logpmf (n_records,) = log(sum_i w_i prod_c P_c,i(k_c) / W) of the records d_settings | d_counts
 * (C, n_records) | d_side (C, n_records) — the JOINT one-step log evidence, not the product of the channels' mixtures —
 * with the term of obe_binomial_records_loglik / obe_poisson_records_loglik per particle, merged as
 * obe_predictive_logpdf merges (a running maximum and a scaled sum: nothing over- or underflows), plus d_constant
 * (n_records,), what no particle changes (sum_c log C(n, k) or -sum_c log k!, the host's).  -inf where the record is
 * impossible for every contributing particle; NaN where W == 0 or the record's data cannot be one.  d_ws as above. */
#define OBE_COUNT_MAX_OUTCOMES 4096
#define OBE_COUNT_MAX_LEVELS 16
#define OBE_COUNT_BINOMIAL 0
#define OBE_COUNT_POISSON 1
OBE_API int64_t obe_count_workspace_bytes(int64_t n_particles, int64_t n_points, int32_t n_channels, int32_t count_max);
OBE_API int obe_count_table(const obe_model* m, int32_t law, const double* d_settings, int64_t ld_s, int64_t n_points,
                    const double* d_side, int64_t ld_side, const double* d_logfact, const double* d_particles,
                    int64_t ld_p, int64_t n_particles, const double* d_weights, int32_t count_max, double* d_pmf,
                    void* d_ws, int64_t ws_bytes, void* stream);
OBE_API int obe_count_tails(const double* d_pmf, int32_t n_channels, int32_t count_max, int64_t n_points,
                    const double* d_counts, int64_t ld_k, double* d_lower, double* d_upper, void* stream);
OBE_API int obe_count_quantiles(const double* d_pmf, int32_t n_channels, int32_t count_max, int64_t n_points,
                        const double* h_levels, int32_t n_levels, double* d_quantiles, void* stream);
OBE_API int obe_count_logpmf(const obe_model* m, int32_t law, const double* d_settings, int64_t ld_s, int64_t n_records,
                     const double* d_counts, int64_t ld_k, const double* d_side, int64_t ld_side,
                     const double* d_constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                     const double* d_weights, double* d_logpmf, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- timing on the launch stream (bench.py roofline leg) ---- */
OBE_API int obe_timer_create(void** timer);
OBE_API int obe_timer_start(void* timer, void* stream);
OBE_API int obe_timer_stop(void* timer, void* stream, float* ms);   /* records, syncs, returns elapsed */
OBE_API int obe_timer_destroy(void* timer);
/* Timing of the dominant sweep kernel inside real cycles: while enabled, every obe_sweep_utility
 * call that returns its result to the host brackets the sweep kernel with two events on its
 * stream and adds the elapsed time to a running total (the events are read after the stream
 * synchronisation the result copy performs anyway).  Returns the total and the number of
 * launches accumulated so far, then: enable > 0 starts a fresh accumulation, enable == 0 stops
 * it, enable < 0 leaves the state alone (read only).  One accumulation per process (per loaded
 * library: a plugin keeps its own), not thread-safe.  bench.py: roofline.achieved. */
OBE_API int obe_sweep_timing(int32_t enable, double* h_total_ms, int64_t* h_launches);
/* Launches only the dominant sweep kernel `iters` times between two events on `stream`
 * and returns the average per-launch duration in ms; iters < 0: -iters isolated launches
 * (the stream is drained before each one), as a measurement cycle issues them.  With OBE_SWEEP_BINS that is the whole
 * pipeline behind the pack, grouping included — a rebuild, whatever obe_sweep_utility_keep() callers keep. */
OBE_API int obe_sweep_kernel_time(const obe_model* m,
                          const double* d_settings, int64_t ld_s, int64_t n_settings,
                          const double* d_particles, int64_t ld_p, int64_t n_particles,
                          const double* d_weights, const double* d_moments, int32_t shifted,
                          void* d_ws, int64_t ws_bytes, int32_t iters, float* h_ms_avg,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OBE_HIP_H */
